"""The lab stamps' slot table (rlvi_amd/csrc/rlvi_stamps.h) as its reader tools/stamps.py sees it: the header parses,
the regions are disjoint and inside the extent, the tools ask only for names that exist, no literal slot is left
outside the header, and a synthetic buffer decodes to the words that were put into it.  No library is loaded."""
import glob
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stamps  # noqa: E402

TOOLS = ["tools/time_parts.py", "tools/estep_sizes.py", "tools/estep_cold.py", "tools/estep_rounds_in_training.py",
         "tools/lab/estep_cold_stamps.py"]


def test_header_parses():
    table, extent = stamps.parse_header()
    assert extent == stamps.EXTENT and table == stamps.TABLE
    # one X(...) line of the list per region: nothing the parser skipped
    text = open(stamps.HEADER).read()
    listed = re.findall(r"^\s*X\((\w+),", text, re.M)
    assert listed == list(table) and len(set(listed)) == len(listed) > 20
    assert all(what.strip() for _, _, what in table.values())
    for name in ("THR_SEQ", "THR_COUNT", "SOLVE_SEQ", "SOLVE_COUNT", "SOLVE_ROUNDS", "FUSED_SEQ", "ENTRY"):
        assert name in table


def test_regions_disjoint_and_inside_extent():
    stamps.check_layout()
    used = np.zeros(stamps.EXTENT, int)
    for first, count, _ in stamps.TABLE.values():
        assert 0 <= first and count >= 1 and first + count <= stamps.EXTENT
        used[first:first + count] += 1
    assert used.max() == 1
    # the overlaps the old numbering had are gone: 64 per-lane words against the kernel's cycle and tick counts,
    # the threshold's block against the solve's sequential stamps, their count and the per-round words
    t = stamps.TABLE
    lanes = range(t["SOLVE_TOTALS_MIN"][0], t["SOLVE_TOTALS_MIN"][0] + 64)
    assert t["SOLVE_TOTALS_MIN"][1] == 64 and t["KERNEL_CYCLES"][0] not in lanes and t["KERNEL_TICKS"][0] not in lanes
    thr = set(range(t["THR_SEQ"][0], t["THR_COUNT"][0] + 1))
    for name in ("SOLVE_SEQ", "SOLVE_COUNT", "SOLVE_ROUNDS"):
        assert not thr & set(range(t[name][0], t[name][0] + t[name][1]))
    # and the checker does catch an overlap and a region past the end
    with pytest.raises(ValueError):
        stamps.check_layout({"A": (0, 8, ""), "B": (7, 2, "")}, 16)
    with pytest.raises(ValueError):
        stamps.check_layout({"A": (10, 8, "")}, 16)


def test_tools_ask_for_names_that_exist():
    asked = 0
    for rel in TOOLS + ["tools/stamps.py"]:
        src = open(os.path.join(ROOT, rel)).read()
        if rel != "tools/stamps.py":
            assert re.search(r"^\s*import stamps\b", src, re.M), rel
        # a region is named by an upper-case string: S.seq("SOLVE_SEQ", "SOLVE_COUNT"), at('ENTRY', 1), st["TJ_SCALE"]
        for name in re.findall(r"""["']([A-Z][A-Z0-9_]{2,})["']""", src):
            if name.startswith("RLVI_"):       # knobs and environment variables
                continue
            assert name in stamps.TABLE, f"{rel} asks for stamp region {name}"
            asked += 1
    assert asked >= 30


def test_no_literal_slot_outside_the_header():
    pats = [re.compile(r"dbg\[\s*\d"), re.compile(r"dbg\[\s*\d+\s*\+")]
    for path in glob.glob(os.path.join(ROOT, "rlvi_amd", "csrc", "*")):
        if os.path.basename(path) == "rlvi_stamps.h" or not os.path.isfile(path):
            continue
        for n, line in enumerate(open(path, errors="replace"), 1):
            assert not any(p.search(line) for p in pats), f"{path}:{n}: {line.strip()}"
    # the tools index the scratch by name only: no slice of the workspace buffer, no word picked by number
    for rel in TOOLS:
        src = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"\braw\[|\bfull\[|ws\w*(\[\d+\])?\.buf\[|debug_scratch_offset", src), rel


def _synthetic():
    rng = np.random.default_rng(7)
    raw = rng.integers(1, 2 ** 63, stamps.EXTENT, dtype=np.int64).astype(np.uint64)     # noise everywhere else
    t = stamps.TABLE

    def put(name, i, v):
        raw[t[name][0] + i] = np.uint64(v)
    return raw, put


def _bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def test_decode_packed_pairs():
    raw, put = _synthetic()
    rn = np.linspace(19.0, 0.001, 64).astype(np.float32)
    rnew = (rn * np.float32(1.03125)).astype(np.float32)
    for lane in range(64):
        put("TJ_NODES", lane, (_bits(rn[lane]) << 32) | _bits(rnew[lane]))
    put("TJ_ACCEPT", 0, (1 << 32) | 17)
    put("TJ_IT_DELTA", 0, (23 << 32) | _bits(2.5e-7))
    put("TJ_SCALE", 0, _bits(0.75))
    put("TJ_TOTALS", 4, int(np.array([1234.5678], np.float64).view(np.uint64)[0]))
    st = stamps.Stamps(raw)
    h, l = st.f32_pair("TJ_NODES")
    assert h.dtype == np.float32 and np.array_equal(h, rn) and np.array_equal(l, rnew)
    acc, it = st.pair("TJ_ACCEPT")
    assert (int(acc[0]), int(it[0])) == (1, 17)
    it, delta = st.pair("TJ_IT_DELTA")
    assert int(it[0]) == 23 and stamps.f32(delta)[0] == np.float32(2.5e-7)
    assert stamps.f32(stamps.lo(st["TJ_SCALE"]))[0] == np.float32(0.75)
    assert st.f64("TJ_TOTALS")[4] == 1234.5678
    assert st.word("TJ_ACCEPT") == (1 << 32) | 17
    # a region is exactly its slots: the neighbours' noise stays out
    assert len(st["TJ_NODES"]) == 64 and len(st["TJ_ACCEPT"]) == 1


def test_decode_sequential_stamps_and_us():
    raw, put = _synthetic()
    t0 = 987_654_321_000
    ticks = [t0, t0 + 150, t0 + 1234, t0 + 100_000]
    for i, v in enumerate(ticks):
        put("SOLVE_SEQ", i, v)
    put("SOLVE_COUNT", 0, len(ticks))
    for i, v in enumerate(ticks[:3]):
        put("THR_SEQ", i, v + 7)
    put("THR_COUNT", 0, 3)
    st = stamps.Stamps(raw)
    seq = st.seq("SOLVE_SEQ", "SOLVE_COUNT")
    assert seq.dtype == np.int64 and list(seq) == ticks
    assert stamps.us(seq) == [0.0, 1.5, 12.34, 1000.0]              # 100 ticks per us, relative to the first
    assert stamps.us(seq, ticks[1]) == [-1.5, 0.0, 10.84, 998.5]   # ... or to a named stamp
    assert stamps.us(ticks[2], t0) == [12.34]
    assert list(st.seq("THR_SEQ", "THR_COUNT")) == [v + 7 for v in ticks[:3]]
    assert stamps.us([]) == []
    # a count beyond the region (a stale or foreign word) is cut to the region
    put("THR_COUNT", 0, 10 ** 6)
    assert len(stamps.Stamps(raw).seq("THR_SEQ", "THR_COUNT")) == stamps.TABLE["THR_SEQ"][1]


def test_decode_rounds_and_short_buffer():
    raw, put = _synthetic()
    for i in range(stamps.TABLE["SOLVE_ROUNDS"][1]):
        put("SOLVE_ROUNDS", i, 0)
    put("SOLVE_ROUNDS", 0, (((24 << 8) | 21) << 32) | _bits(3.0e-4))
    put("SOLVE_ROUNDS", 1, (((24 << 8) | 22) << 32) | _bits(0.0) | 0)     # delta 0.0 of an accepted round ...
    st = stamps.Stamps(raw)
    assert stamps.rounds(st) == [(24, 21, float(np.float32(3.0e-4))), (24, 22, 0.0)]   # ... still counts: Ke, it != 0
    # a workspace of the product library is shorter than the table: the rest reads as zeros
    short = stamps.Stamps(raw[:300])
    assert short.raw.size == stamps.EXTENT and short.word("CHAIN_SEQ") == 0 and stamps.rounds(short) == stamps.rounds(st)
