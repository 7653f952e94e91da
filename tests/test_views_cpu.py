"""tests/views.py on CPU tensors: every kind's offset, strides and poison, and expected_vector on hand-written cases."""
import numpy as np
import pytest
import torch

from views import COL_PAD, KINDS, expected_vector, layout, outside, place

B, C = 5, 12
DTYPES = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2}
# kind -> (element offset of the view, row pitch), written out by hand for [5, 12]
PLACES = {"dense": (0, 12), "rows+1": (12, 12), "elem+1": (1, 12), "elem+2": (2, 12), "elem+4": (4, 12),
          "pitch+1": (0, 13), "pitch+2": (0, 14), "pitch+4": (0, 16), "col+1": (1, 20)}


def test_the_table_names_every_kind():
    assert set(PLACES) == set(KINDS) and len(KINDS) == 9 and COL_PAD == 8


@pytest.mark.parametrize("dtype", list(DTYPES), ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_offset_strides_and_poison(kind, dtype):
    s = DTYPES[dtype]
    a = (torch.arange(B * C, dtype=torch.float32).reshape(B, C) - 7).to(dtype)
    view, buf = place(torch, a, kind, float("nan"), "cpu")
    off, pitch = PLACES[kind]
    assert view.dtype == dtype and buf.dtype == dtype and buf.dim() == 1 and buf.is_contiguous()
    assert buf.data_ptr() % 64 == 0                                   # (a fresh allocation)
    assert view.shape == (B, C) and view.stride() == (pitch, 1)
    assert view.data_ptr() - buf.data_ptr() == off * s
    assert layout(kind, B, C)[1:] == (off, pitch)
    assert torch.equal(view, a)
    assert view.is_contiguous() == (pitch == C)
    # the poison everywhere outside the view, and nowhere inside it
    m = outside(torch, view, buf)
    assert int(m.sum()) == buf.numel() - B * C
    assert torch.isnan(buf[m]).all() and not torch.isnan(buf[~m]).any()
    assert (int(m.sum()) == 0) == (kind == "dense")
    # the view shares the buffer: a write through it lands at offset + row * pitch + column
    view[3, 2] = 99.0
    assert float(buf[off + 3 * pitch + 2]) == 99.0


def test_a_finite_poison_is_kept_bit_for_bit():
    a = torch.zeros(B, C)
    view, buf = place(torch, a, "col+1", 7.0, "cpu")
    m = outside(torch, view, buf)
    assert torch.equal(buf[m].view(torch.int32), torch.full((B * COL_PAD,), 7.0).view(torch.int32))
    view, buf = place(torch, np.ones((B, C), np.float32), "rows+1", 7.0, "cpu")       # (a numpy array goes in too)
    assert buf[:C].eq(7.0).all() and buf[C:].eq(1.0).all()


def test_rows_plus_one_is_what_chunk_gives():
    whole = torch.zeros(2 * B, 10)
    second = whole.chunk(2)[1]
    view, buf = place(torch, torch.zeros(1, 10), "rows+1", 0.0, "cpu")
    assert (second.data_ptr() - whole.data_ptr()) == B * 40
    assert view.data_ptr() - buf.data_ptr() == 40                    # row 1 of a [*, 10] fp32 batch: +40 bytes
    view, buf = place(torch, torch.zeros(1, 101, dtype=torch.bfloat16), "rows+1", 0.0, "cpu")
    assert view.data_ptr() - buf.data_ptr() == 202                   # ... of a [*, 101] bf16 batch: +202


def test_expected_vector_on_hand_written_cases():
    base = 1 << 20
    ev = expected_vector
    assert ev(4, 100, [(base, 100)]) == 4 and ev(2, 104, [(base, 104)]) == 8
    assert ev(4, 100, [(base + 8, 100)]) == 2                        # fp32, C = 100 at +8 bytes
    assert ev(2, 104, [(base + 8, 104)]) == 4                        # bf16, C = 104 at +8 bytes
    assert ev(4, 100, [(base + 4, 100)]) == 1 and ev(2, 104, [(base + 2, 104)]) == 1
    assert ev(2, 104, [(base + 4, 104)]) == 2 and ev(2, 104, [(base + 16, 104)]) == 8
    for c in (1, 7, 37, 101, 1001):                                  # any odd C
        assert ev(4, c, [(base, c)]) == 1 and ev(2, c, [(base, c + 1)]) == 1
    assert ev(4, 100, [(base, 102)]) == 2 and ev(4, 100, [(base, 101)]) == 1 and ev(4, 100, [(base, 104)]) == 4
    assert ev(2, 100, [(base, 100)]) == 4 and ev(2, 102, [(base, 102)]) == 2     # 2-byte rows that 8 does not divide
    # every block counts: the second (a gradient) alone narrows the vector; None is skipped
    assert ev(4, 100, [(base, 100), (base + 4096, 100)]) == 4
    assert ev(4, 100, [(base, 100), (base + 4, 100)]) == 1
    assert ev(4, 100, [(base, 100), (base, 102)]) == 2
    assert ev(4, 100, [(base + 8, 104), None, (base, 101)]) == 1
    assert ev(4, 100, [(base, 100), None]) == 4
    assert ev(2, 104, [(base + 8, 104), (base + 4, 104)]) == 2


@pytest.mark.parametrize("dtype", list(DTYPES), ids=str)
def test_expected_vector_on_placed_tensors(dtype):
    s = DTYPES[dtype]
    vmax = 16 // s
    want = {"dense": vmax, "rows+1": vmax, "elem+1": 1, "elem+2": 2, "elem+4": 4, "pitch+1": 1, "pitch+2": 2,
            "pitch+4": 4, "col+1": 1}
    a = torch.zeros(6, 104, dtype=dtype)                             # 104 * s is a multiple of 16: rows+1 stays aligned
    for kind in KINDS:
        view, _ = place(torch, a, kind, 0.0, "cpu")
        assert expected_vector(s, 104, [view]) == want[kind], kind
    a = torch.zeros(6, 100, dtype=dtype)                             # 100 elements: 400 or 200 bytes a row
    view, _ = place(torch, a, "rows+1", 0.0, "cpu")
    assert expected_vector(s, 100, [view]) == 4
    a = torch.zeros(6, 10, dtype=dtype)
    view, _ = place(torch, a, "rows+1", 0.0, "cpu")                  # +40 / +20 bytes
    assert expected_vector(s, 10, [view]) == 2
    dense, _ = place(torch, a, "dense", 0.0, "cpu")
    assert expected_vector(s, 10, [dense, view]) == 2 and expected_vector(s, 10, [dense, None]) == 2
