"""Reader of the lab builds' stamp table (rlvi_amd/csrc/rlvi_stamps.h).

The header's X-macro list is the only table: this module parses it, so a region moved there moves here.

    import stamps
    st = stamps.read(ws)                 # after a -DRLVI_STAMPS=1 library ran with RLVI_TJ_DEBUG=1 / RLVI_THR_DEBUG=1
    seq = st.seq("SOLVE_SEQ", "SOLVE_COUNT")        # the sequential stamps that were taken, int64 ticks
    stamps.us(seq, seq[0])                          # ... as us since the first one
    hi, lo = st.pair("TJ_NODES")                    # packed (hi, lo) 32-bit words of every slot
    stamps.f32(lo)                                  # ... read as fp32

Needs numpy only; read() and clear() import rlvi_amd.ops for the table's offset in the workspace."""
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rlvi_amd", "csrc", "rlvi_stamps.h")
TICKS_PER_US = 100.0            # the wall clock the stamps are taken from runs at 100 MHz


def parse_header(path=HEADER):
    """({name: (first, count, what)}, extent in slots) of the header's X(name, first, count, "what") lines."""
    text = open(path).read()
    table = {}
    for name, first, count, what in re.findall(r'^\s*X\(\s*(\w+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*"([^"]*)"\s*\)', text, re.M):
        if name in table:
            raise ValueError(f"{path}: region {name} listed twice")
        table[name] = (int(first), int(count), what)
    m = re.search(r"constexpr\s+int\s+STAMP_EXTENT\s*=\s*(\d+)\s*;", text)
    if not table or not m:
        raise ValueError(f"{path}: no stamp table found")
    return table, int(m.group(1))


TABLE, EXTENT = parse_header()


def check_layout(table=TABLE, extent=EXTENT):
    """Raises if two regions overlap or one leaves the extent (the header's static_assert, for the readers)."""
    spans = sorted((first, first + count, name) for name, (first, count, _) in table.items())
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        if b0 < a1:
            raise ValueError(f"stamp regions {an} [{a0}, {a1}) and {bn} [{b0}, {b1}) overlap")
    for a0, a1, an in spans:
        if a0 < 0 or a1 <= a0 or a1 > extent:
            raise ValueError(f"stamp region {an} [{a0}, {a1}) is empty or outside the table's {extent} slots")


# ---- decoders
def hi(words):
    return (np.asarray(words, np.uint64) >> np.uint64(32)).astype(np.uint32)


def lo(words):
    return (np.asarray(words, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def f32(words32):
    return np.asarray(words32, np.uint32).view(np.float32)


def us(ticks, origin=None, digits=2):
    """Wall-clock ticks as us relative to the stamp `origin` (default: the first of them)."""
    ticks = [int(t) for t in np.atleast_1d(ticks)]
    origin = int(origin) if origin is not None else (ticks[0] if ticks else 0)
    return [round((t - origin) / TICKS_PER_US, digits) for t in ticks]


class Stamps:
    """The table as named arrays over one uint64 buffer (shorter buffers read as zeros past their end)."""

    def __init__(self, raw):
        raw = np.asarray(raw, np.uint64)
        self.raw = np.zeros(EXTENT, np.uint64)
        self.raw[:min(EXTENT, raw.size)] = raw[:EXTENT]

    def __getitem__(self, name):
        first, count, _ = TABLE[name]
        return self.raw[first:first + count]

    def word(self, name, i=0):
        return int(self[name][i])

    def ticks(self, name):
        return self[name].astype(np.int64)

    def seq(self, name, count_name):
        """The sequential stamps of region `name` that were taken (their number is in `count_name`), int64."""
        n = min(self.word(count_name), TABLE[name][1])
        return self.ticks(name)[:n]

    def pair(self, name):
        return hi(self[name]), lo(self[name])

    def f32_pair(self, name):
        h, l = self.pair(name)
        return f32(h), f32(l)

    def f64(self, name):
        return self[name].view(np.float64)


def rounds(st):
    """[(Ke, it, delta)] of the rounds a solve took: the non-zero words of SOLVE_ROUNDS."""
    keit, delta = st.pair("SOLVE_ROUNDS")
    return [(int(k) >> 8, int(k) & 0xFF, float(d)) for k, d, x in zip(keit, f32(delta), st["SOLVE_ROUNDS"]) if x]


def _span(ws, name=None):
    from rlvi_amd import ops
    off = ops.debug_scratch_offset()
    first, count = (0, EXTENT) if name is None else TABLE[name][:2]
    return ws.buf[off + 8 * first:off + 8 * (first + count)]


def read(ws):
    """The stamps a launch left in the workspace `ws` (synchronises)."""
    return Stamps(_span(ws).cpu().numpy().view(np.uint64))


def clear(ws, name=None):
    """Zeroes one region (or the whole table) in the workspace, for readers that test a slot for 0."""
    _span(ws, name).zero_()
