"""Shared pieces of the large-extent tests (test_large_extents_cpu.py, test_large_extents_gpu.py; DESIGN.md "Addressing
limits"): operands past 2 GiB, 4 GiB and 2^31 elements.

The four boundaries, measured from an operand's base:

  B31  2^31 bytes      31-bit buffer descriptors (make_rsrc clamps num_records to 0x7fffffff), signed 32-bit byte offsets
  B32  2^32 bytes      unsigned 32-bit byte offsets, unsigned(...) narrowings
  E31  2^31 elements   `int` element indices (2^33 bytes of fp32)
  E32  2^32 elements   the high word of lamp_dropout's 64-bit counter (2^34 bytes)

A case crosses a boundary when live data and checked results lie on both sides of it within one operand.

BigArena is redzone_common.Arena's contract at these sizes without its footprint (Arena clones a pristine copy and
torch.cat()s in check(): three times the bytes):

  * one device allocation; every operand starts 256-byte aligned, is exactly as long as asked, and has ZONE bytes of sentinel
    on either side;
  * BELOW the first operand lies a landing zone of sentinel at least as long as the largest operand.  An offset truncated
    to 32 bits and sign-extended is at most 2^31 elements below where it should be, i.e. at most one operand's length
    below the operand's base when the operand is what made the offset large; an offset wrapped as unsigned lands inside the
    operand itself.  Either way a wrong access stays in memory the test owns and shows as a failed assertion: a sentinel
    read (NaN under FILL_NAN), a sentinel left in an output, or a changed word in the landing zone;
  * sentinel regions are checked chunk by chunk on the device (an integer compare against the fill word, at most CHUNK
    bytes at a time); nothing large is copied to the host.

References are computed for row windows only (windows()), in fp64 on the CPU, from rows copied back.  Operands whose
output rows do not depend on the row's position are built periodic along rows (fill_periodic_rows) with a period that is
no multiple of any tile height, and the whole output is checked bit-periodic on the device (assert_bit_periodic).

The int32 mutants at the end restate the pointer-based kernels' index arithmetic with the index narrowed to `int`, for the
CPU file's "would this case fail under the bug it targets" checks."""
import torch

from redzone_common import ALIGN, FILL_BIG, FILL_NAN, FILLS, ZONE, _i32   # noqa: F401  (re-exported)

B31 = 1 << 31
B32 = 1 << 32
E31 = (1 << 31) * 4      # byte offsets of the element boundaries of an fp32 operand
E32 = (1 << 32) * 4
BOUNDARIES = (('B31', B31), ('B32', B32), ('E31', E31), ('E32', E32))

CHUNK = 256 << 20        # bytes per device-side compare / fill
PERIOD = 4099            # rows per period: prime, so no multiple of a tile height (16 .. 256) or of a 4-row workgroup
WINDOW = 128             # rows on either side of a boundary
GIB = 1 << 30
BUDGET = 40 * GIB        # no case may need more, torch temporaries included
TEMP = 5 * CHUNK         # allowance for what the chunked fills / compares hold at once (a block of periods, masks, gathers)


def align_up(n, a=ALIGN):
    return (int(n) + a - 1) // a * a


# ---------------------------------------------------------------------------------------------------------------- layout
def layout(operands):
    """operands: [(name, nbytes)] -> ({name: (begin, end)}, total bytes, landing-zone bytes).  Pure Python integers."""
    landing = align_up(max([n for _, n in operands] + [0]))
    pos, spans = landing, {}
    for name, nbytes in operands:
        a = align_up(pos + ZONE)
        spans[name] = (a, a + int(nbytes))
        pos = a + int(nbytes)
    return spans, align_up(pos + ZONE), landing


def need_bytes(operands, extra=0):
    """Peak device bytes of a case: the arena, this file's chunked temporaries, and whatever else the case allocates."""
    return layout(operands)[1] + ALIGN + TEMP + int(extra)


def require_memory(need):
    """The one permitted skip: less free device memory than need + 2 GiB.  A need beyond the budget is the case's own bug."""
    import pytest
    assert need <= BUDGET, 'case needs %d bytes, the budget is %d' % (need, BUDGET)
    free, _total = torch.cuda.mem_get_info()
    if free < need + 2 * GIB:
        pytest.skip('free device memory %d < need %d + 2 GiB' % (free, need))


class BigArena(object):
    def __init__(self, device, fill, operands):
        """operands: [(name, nbytes)] in address order.  Everything starts as the sentinel word."""
        self.device, self.fill = device, fill
        self.spans, self.total, self.landing = layout(operands)
        self._raw = torch.empty(self.total + ALIGN, dtype=torch.uint8, device=device)
        skew = (-self._raw.data_ptr()) % ALIGN
        self.mem = self._raw[skew:skew + self.total]
        words = self.mem.view(torch.int32)
        for a in range(0, words.numel(), CHUNK // 4):
            words[a:a + CHUNK // 4].fill_(_i32(fill))

    def _sync(self):
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)

    def free(self):
        self.mem = self._raw = None

    def view(self, name, dtype=torch.float32, shape=None):
        a, b = self.spans[name]
        v = self.mem[a:b].view(dtype)
        return v if shape is None else v.view(shape)

    def ptr(self, name):
        return self.mem.data_ptr() + self.spans[name][0]

    def nbytes(self, name):
        a, b = self.spans[name]
        return b - a

    # ---- checks, all on the device and chunked
    def _first_bad(self, a, b):
        """First byte offset in [a, b) (4-byte aligned bounds) whose word is not the sentinel, or -1."""
        words, sent = self.mem.view(torch.int32), _i32(self.fill)
        for c in range(a // 4, b // 4, CHUNK // 4):
            bad = words[c:min(c + CHUNK // 4, b // 4)] != sent
            if bool(bad.any()):
                return (c + int(bad.nonzero()[0])) * 4
        return -1

    def _where(self, off):
        """Where a byte of the arena lies, in words: its distance to the operands on either side."""
        msg = ['arena offset %d' % off]
        if off < self.landing:
            msg.append('landing zone, %d bytes below the first operand' % (min(a for a, _ in self.spans.values()) - off))
        ends = [(b, name) for name, (_, b) in self.spans.items() if b <= off]
        starts = [(a, name) for name, (a, _) in self.spans.items() if a > off]
        if ends:
            end, name = max(ends)
            msg.append('%d bytes past the end of %r' % (off - end, name))
        if starts:
            start, name = min(starts)
            msg.append('%d bytes before %r' % (start - off, name))
        return ', '.join(msg)

    def check_zones(self):
        """No sentinel word outside the operands changed: the landing zone and every red zone."""
        self._sync()
        pos = 0
        for name, (a, b) in sorted(self.spans.items(), key=lambda kv: kv[1]):
            lo, hi = pos, a // 4 * 4
            off = self._first_bad(lo, hi)
            assert off < 0, 'a word outside the operands changed: ' + self._where(off)
            pos = (b + 3) // 4 * 4
        off = self._first_bad(pos, self.total)
        assert off < 0, 'a word outside the operands changed: ' + self._where(off)

    def check_written(self, name):
        """No sentinel word is left in an operand the call must have written in full."""
        self._sync()
        words, sent = self.view(name, torch.int32), _i32(self.fill)
        for c in range(0, words.numel(), CHUNK // 4):
            left = words[c:c + CHUNK // 4] == sent
            assert not bool(left.any()), ('%d words of output %r never written in one chunk, first at word %d'
                                          % (int(left.sum()), name, c + int(left.nonzero()[0])))

    def check_untouched(self, name):
        """Every word of the operand still is the sentinel (a refused call wrote nothing)."""
        self._sync()
        a, b = self.spans[name]
        off = self._first_bad(a, b // 4 * 4)
        assert off < 0, 'refused call wrote into %r at byte %d' % (name, off - a)


# ------------------------------------------------------------------------------------------------------------- windows
def crossings(nbytes):
    """Names of the boundaries that lie strictly inside an operand of nbytes."""
    return [name for name, at in BOUNDARIES if at < nbytes]


def windows(rows, row_bytes, width=WINDOW):
    """Row ranges [(r0, r1)] to hold against fp64: the first `width` rows, `width` rows on either side of every boundary the
    operand crosses (the row that straddles it included), and the last width + (rows % width) rows: the ragged tail of any
    tile height up to `width`.  Merged and sorted."""
    rows, row_bytes = int(rows), int(row_bytes)
    want = [(0, min(width, rows))]
    for _, at in BOUNDARIES:
        if at < rows * row_bytes:
            r = at // row_bytes
            want.append((max(r - width, 0), min(r + width + 1, rows)))
    want.append((max(rows - width - rows % width, 0), rows))
    want.sort()
    out = [want[0]]
    for a, b in want[1:]:
        if a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def window_rows(wins):
    """All row indices of the windows, as one int64 tensor."""
    return torch.cat([torch.arange(a, b, dtype=torch.int64) for a, b in wins])


def take_rows(view2d, wins):
    """The windows' rows of a device [rows, cols] view, copied to the CPU (small)."""
    return torch.cat([view2d[a:b] for a, b in wins]).cpu()


# ------------------------------------------------------------------------------------------------- periodic operands
def fill_periodic_rows(view2d, period):
    """view2d[r] = period[r % P] for every row, from blocks of whole periods of at most CHUNK bytes (period: [P, cols],
    any device)."""
    rows, cols = view2d.shape
    P = period.shape[0]
    period = period.to(view2d.device, view2d.dtype)
    k = max(1, min(CHUNK // (P * cols * view2d.element_size()), (rows + P - 1) // P))
    block = period.repeat(k, 1)
    for r in range(0, rows, k * P):
        n = min(k * P, rows - r)
        view2d[r:r + n].copy_(block[:n])


def periodic_rows(period, rows_idx):
    """What fill_periodic_rows put into the given rows (CPU restatement from the generator: the input check)."""
    return period.cpu()[rows_idx % period.shape[0]]


def assert_bit_periodic(view2d, P, what):
    """view2d[r + P] == view2d[r] bit for bit over the whole length, by chunked integer compares on the device."""
    rows, cols = view2d.shape
    w = view2d.view(torch.int32) if view2d.element_size() == 4 else view2d
    step = max(1, CHUNK // (cols * 4))
    for r in range(0, rows - P, step):
        n = min(step, rows - P - r)
        same = w[r:r + n] == w[r + P:r + P + n]
        if not bool(same.all()):
            bad = (~same).nonzero()[0].tolist()
            raise AssertionError('%s: row %d differs from row %d at column %d: not periodic'
                                 % (what, r + bad[0] + P, r + bad[0], bad[1]))


def assert_rows_equal_generator(view2d, period, wins, what):
    """An input must come back bit-unchanged: its windows against the generator that produced them, and (cheap, on the
    device) the whole operand still periodic."""
    got = take_rows(view2d, wins)
    want = periodic_rows(period.to(view2d.dtype), window_rows(wins))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), '%s: input changed' % what
    assert_bit_periodic(view2d, period.shape[0], what + ' (input)')


def checksum(view1d):
    """A 64-bit wrap-around sum of the words of a device operand, chunked: an input check taken before and after a call."""
    words, total = view1d.view(torch.int32), 0
    for c in range(0, words.numel(), CHUNK // 4):
        total = (total + int(words[c:c + CHUNK // 4].sum(dtype=torch.int64))) & ((1 << 64) - 1)
    return total


# ------------------------------------------------------------------------------------ int32 mutants (CPU, windows only)
def narrow_i32(x):
    """x (Python int or int64 tensor) truncated to 32 bits and sign-extended: what `int(...)` makes of a 64-bit index."""
    return ((x + (1 << 31)) & 0xffffffff) - (1 << 31)


def narrow_u32(x):
    """x truncated to 32 bits, zero-extended: what `unsigned(...)` makes of it."""
    return x & 0xffffffff


def mutant_source_rows(rows_idx, cols, narrow=narrow_i32, unit=1):
    """The row a kernel would read for each of rows_idx if it formed the offset row * cols * unit in 32 bits (unit 1: an
    element index, 4: a byte offset): (narrowed offset) // (cols * unit), and -1 where the narrowed offset is negative --
    below the operand's base, in the landing zone: a sentinel read."""
    off = narrow(rows_idx * (int(cols) * int(unit)))
    return torch.where(off < 0, torch.full_like(off, -1), off // (int(cols) * int(unit)))


def mutant_periodic_rows(period, rows_idx, cols=None, narrow=narrow_i32, unit=1):
    """The rows the mutant of mutant_source_rows reads from a periodic operand; NaN rows where it reads the sentinel."""
    cols = period.shape[1] if cols is None else cols
    src = mutant_source_rows(rows_idx, cols, narrow, unit)
    out = period.cpu()[src.clamp(min=0) % period.shape[0]].clone()
    out[src < 0] = float('nan')
    return out


def mutant_keep_mask(n, p, seed, start, narrow=narrow_i32):
    """lamp_dropout's keep mask with the element index narrowed to 32 bits before it is split into the two words mix32 takes
    (lamp_amd/_native.py: dropout_keep_mask is the true restatement)."""
    e = narrow(torch.arange(int(start), int(start) + int(n), dtype=torch.int64))
    m32 = 0xffffffff
    h = ((e & m32) ^ ((((e >> 32) & m32) * 0x9E3779B9) & m32) ^ (int(seed) & m32)) & m32
    h = h ^ (h >> 16)
    h = (h * 0x7feb352d) & m32
    h = h ^ (h >> 15)
    h = (h * 0x846ca68b) & m32
    h = h ^ (h >> 16)
    thr = min(int(float(torch.tensor(p, dtype=torch.float32)) * 4294967296.0), 4294967295)
    return h >= thr


# ------------------------------------------------------------------------------------------- shapes shared by both files
# (rows, cols) of the cases, so that the CPU file can show at window indices that each would fail under its mutant.
LN_E31 = ((1 << 22) + 64 + 37, 512)            # M * d crosses E31 (and B31, B32)
SOFTMAX_E31 = (7158279 + 300, 300)             # rows * lk crosses E31: 2^31 / 300 = 7158278.8
BCE_B32 = (1168371 + 2 * WINDOW + 37, 919)     # n * L * 4 crosses B32: 2^30 / 919 = 1168370.9
COLSUM_TALL = ((1 << 20) + 101, 1028)          # M * N * 4 crosses B32
DIAG_B32 = (4099, 520, 512)                    # B, L, d: B * L * d * 4 crosses B32
DROPOUT_N = (1 << 32) + (1 << 20) + 3
OPTIM_NUMEL = ((1 << 30) + 4096 + 3, 4095, 1001)
FLAT_WINDOW = 8192                             # elements either side of a boundary of a flat operand (two optimizer chunks)
