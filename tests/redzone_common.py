"""One device allocation carved into exactly-sized buffers with sentinel red zones between them (test_buffer_contracts_gpu.py).

The ordinary wrappers cannot see a store that leaves its buffer: lamp_amd/_native.py: workspace() allocates `nbytes + 256`
and only grows, and outputs are torch tensors inside the caching allocator's blocks, so a ragged-edge store one row or one
tile past M, N, lq or lk lands in live memory -- neither a fault nor a wrong value in the tensor being compared.  An Arena
hands the library raw pointers into memory it owns wholly:

  * every buffer starts 256-byte aligned (torch's own alignment, so the library's alignment-dependent routing is the same)
    and is exactly as many bytes long as include/lamp_hip.h documents; nothing rounds it up;
  * at least ZONE bytes of sentinel lie before and after each buffer.  64 KiB is a choice, not a measurement: a whole stray
    tile row of any kernel here (64 rows x 64 columns x 4 bytes = 16 KiB) lands inside a zone;
  * red zones, workspaces and outputs start as one 32-bit sentinel word repeated: FILL_NAN, a quiet NaN with a payload, told
    apart by an integer compare from the 0x7FC00000 a fully masked attention row produces, or FILL_BIG, a large finite
    value (~1e30).  A result that differs between the two fills depends on bytes outside the contract.

check() after the call asserts that every byte outside the writable buffers -- red zones AND inputs -- is unchanged, that
the padding between the rows of a strided output still holds the sentinel, and that no sentinel word is left in any
element an output is documented to receive."""
import torch

ZONE = 64 * 1024
ALIGN = 256
FILL_NAN = 0x7FC00DED
FILL_BIG = 0x7149F2CA   # ~1e30 as a float
FILLS = (FILL_NAN, FILL_BIG)


def _i32(word):
    return word - (1 << 32) if word >= (1 << 31) else word


def bits(t):
    """The bit pattern of a tensor as a contiguous integer tensor (NaN == NaN, -0.0 != 0.0)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def bit_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class Arena(object):
    def __init__(self, device, fill, capacity=32 << 20):
        assert capacity % 4 == 0
        self.device, self.fill = device, fill
        self._raw = torch.empty(capacity + ALIGN, dtype=torch.uint8, device=device)
        skew = (-self._raw.data_ptr()) % ALIGN
        self.mem = self._raw[skew:skew + capacity]
        self.mem.view(torch.int32).fill_(_i32(fill))
        self._pristine = self.mem.clone()    # what every byte that is not writable must still hold after the call
        self._end = 0                        # first byte not yet given out
        self._writable = []                  # (begin, end, name): outputs, workspaces, in-place operands
        self._outputs = []                   # (name, tensor view of the elements that must be written, exempt)
        self._padding = []                   # (name, tensor view that must still hold the sentinel)
        self._names = []                     # (begin, end, name) of every buffer, for messages

    # ---- carving
    def _carve(self, nbytes, name):
        nbytes = int(nbytes)
        a = (self._end + ZONE + ALIGN - 1) // ALIGN * ALIGN
        if a + nbytes + ZONE > self.mem.numel():
            raise RuntimeError('arena of %d bytes is too small for %s (%d bytes at %d)' % (self.mem.numel(), name, nbytes, a))
        self._end = a + nbytes
        self._names.append((a, a + nbytes, name))
        return a

    def _view(self, a, shape, dtype, ld=None):
        item = torch.empty((), dtype=dtype).element_size()
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        if ld is None:
            return self.mem[a:a + n * item].view(dtype).view(shape)
        assert len(shape) == 2 and ld >= shape[1]
        span = ((shape[0] - 1) * ld + shape[1])
        return self.mem[a:a + span * item].view(dtype).as_strided(shape, (ld, 1))

    @staticmethod
    def _span(shape, dtype, ld):
        item = torch.empty((), dtype=dtype).element_size()
        n = 1
        for s in shape:
            n *= int(s)
        if ld is not None:
            n = (int(shape[0]) - 1) * int(ld) + int(shape[1])
        return n * item

    def _pad_view(self, a, shape, dtype, ld):
        """The (rows - 1) x (ld - cols) words between the rows of a strided buffer."""
        if ld is None or ld == int(shape[1]) or int(shape[0]) < 2:
            return None
        rows, cols = int(shape[0]), int(shape[1])
        item = torch.empty((), dtype=dtype).element_size()
        flat = self.mem[a:a + ((rows - 1) * ld + cols) * item].view(dtype)
        return flat.as_strided((rows - 1, ld - cols), (ld, 1), flat.storage_offset() + cols)   # the offset is the storage's

    def inp(self, data, name, ld=None):
        """An input: `data` (any device) copied into an exactly-sized buffer, rows `ld` elements apart when given (the padding
        keeps the sentinel).  It must come back bit-unchanged."""
        data = data.detach()
        a = self._carve(self._span(data.shape, data.dtype, ld), name)
        v = self._view(a, data.shape, data.dtype, ld)
        v.copy_(data)
        b = self._names[-1][1]
        self._pristine[a:b].copy_(self.mem[a:b])
        return v

    def out(self, shape, name, dtype=torch.float32, ld=None, exempt=False):
        """An output, sentinel-filled.  Every element must have been written by check() (exempt: the header says it may not
        be); the padding of a strided one must not."""
        a = self._carve(self._span(shape, dtype, ld), name)
        v = self._view(a, shape, dtype, ld)
        self._writable.append((a, self._names[-1][1], name))
        if not exempt:
            self._outputs.append((name, v))
        pad = self._pad_view(a, shape, dtype, ld)
        if pad is not None:
            self._padding.append((name, pad))
        return v

    def inout(self, data, name, ld=None):
        """An operand the call updates in place (accumulate, y == x): holds `data`, may change; strided padding may not."""
        data = data.detach()
        a = self._carve(self._span(data.shape, data.dtype, ld), name)
        v = self._view(a, data.shape, data.dtype, ld)
        v.copy_(data)
        self._writable.append((a, self._names[-1][1], name))
        pad = self._pad_view(a, data.shape, data.dtype, ld)
        if pad is not None:
            self._padding.append((name, pad))
        return v

    def scratch(self, nbytes, name):
        """A workspace of exactly nbytes (0: a valid, zone-surrounded pointer to no bytes), sentinel-filled, any content after."""
        a = self._carve(nbytes, name)
        self._writable.append((a, a + int(nbytes), name))
        return self.mem[a:a + int(nbytes)]

    @staticmethod
    def ptr(t):
        return 0 if t is None else t.data_ptr()

    # ---- checking
    def _sync(self):
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)

    def _where(self, off):
        for a, b, name in self._names:
            if a <= off < b:
                return 'inside input %r at byte %d of %d' % (name, off - a, b - a)
        before = [(off - b, name) for a, b, name in self._names if b <= off]
        after = [(a - off, name) for a, b, name in self._names if a > off]
        msg = []
        if before:
            d, name = min(before)
            msg.append('%d bytes past the end of %r' % (d, name))
        if after:
            d, name = min(after)
            msg.append('%d bytes before %r' % (d, name))
        return 'red zone, ' + ', '.join(msg)

    def untouched(self):
        """True when not one byte of the arena, writable buffers included, differs from its state before the call."""
        self._sync()
        return torch.equal(self.mem, self._pristine)

    def check(self):
        self._sync()
        keep, pos = [], 0
        for a, b, _ in sorted(self._writable):
            if a > pos:
                keep.append((pos, a))
            pos = max(pos, b)
        keep.append((pos, self.mem.numel()))
        now = torch.cat([self.mem[a:b] for a, b in keep])
        was = torch.cat([self._pristine[a:b] for a, b in keep])
        if not torch.equal(now, was):
            idx = int((now != was).nonzero()[0])
            n_bad = int((now != was).sum())
            for a, b in keep:
                if idx < b - a:
                    off = a + idx
                    break
                idx -= b - a
            raise AssertionError('%d bytes outside the writable buffers changed; first at arena offset %d: %s'
                                 % (n_bad, off, self._where(off)))
        sent = _i32(self.fill)
        for name, pad in self._padding:
            if pad.element_size() == 4:
                bad = bits(pad) != sent
                assert not bool(bad.any()), 'row padding of %r overwritten at %s' % (name, bad.nonzero()[0].tolist())
        for name, v in self._outputs:
            if v.element_size() != 4:
                continue
            left = bits(v) == sent
            assert not bool(left.any()), ('%d elements of output %r never written, first at %s'
                                          % (int(left.sum()), name, left.nonzero()[0].tolist()))
