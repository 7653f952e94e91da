"""[B, C] blocks placed as tensor views, and the vector width a row kernel may use on them (torch only where a tensor
is handed in; a helper, not a test module).

Every kernel that reads a [B, C] block picks its vector width on the host from C, the row pitch and the block's
base address (rlvi_common.h, vec_fits: "its row pitch (in elements) a multiple of v and its base pointer
v * sizeof(T)-byte aligned").  A fresh allocation is 256-byte aligned, so only a view moves the base or the pitch:

  kind      layout                                        effect (s = element size)
  dense     a fresh tensor                                the control
  rows+1    buf[1:] of a dense [B + 1, C]                 what chunk / split along the batch gives: base at +C * s bytes
  elem+k    flat[k : k + B * C].view(B, C), k = 1, 2, 4   dense, base at +k * s
  pitch+p   wide[:, :C] of [B, C + p], p = 1, 2, 4        base aligned, pitch not
  col+1     wide[:, 1 : 1 + C] of [B, C + 8]              the pitch keeps its alignment, base at +s

place() fills everything around the view with a poison value, so that a kernel that reads a neighbour (NaN) or writes
one (a bit pattern to compare afterwards) shows.
"""

KINDS = ("dense", "rows+1", "elem+1", "elem+2", "elem+4", "pitch+1", "pitch+2", "pitch+4", "col+1")
COL_PAD = 8


def layout(kind, B, C):
    """(elements of the buffer, element offset of the view, row pitch of the view) of a kind."""
    if kind == "dense":
        return B * C, 0, C
    if kind == "rows+1":
        return (B + 1) * C, C, C
    head, _, n = kind.partition("+")
    n = int(n)
    if head == "elem":
        return B * C + 2 * n, n, C         # (n elements of poison on either side)
    if head == "pitch":
        return B * (C + n), 0, C + n
    if head == "col" and n == 1:
        return B * (C + COL_PAD), 1, C + COL_PAD
    raise ValueError(kind)


def place(torch, a, kind, poison, device):
    """(view, buffer): the view holds the [B, C] tensor or array `a` (its dtype kept), every other element of the 1-D
    buffer holds `poison`.  The buffer is a fresh allocation; the view shares its memory."""
    if not torch.is_tensor(a):
        a = torch.from_numpy(a)
    B, C = a.shape
    total, off, pitch = layout(kind, B, C)
    buf = torch.full((total,), poison, dtype=a.dtype, device=device)
    view = buf.as_strided((B, C), (pitch, 1), off)
    view.copy_(a)
    return view, buf


def outside(torch, view, buf):
    """Bool mask over the buffer's elements: True where the view does not reach."""
    B, C = view.shape
    off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    m = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    m.as_strided((B, C), (view.stride(0), 1), off).fill_(False)
    return m


def expected_vector(elem_size, C, blocks):
    """The widest v of {16 / elem_size, 4, 2, 1} that divides C and, for every block -- a tensor, or a
    (byte address, pitch in elements) pair -- its pitch and its address in elements."""
    terms = [b if isinstance(b, tuple) else (b.data_ptr(), b.stride(0)) for b in blocks if b is not None]
    fits = lambda v: C % v == 0 and all(ld % v == 0 and (p // elem_size) % v == 0 for p, ld in terms)
    return next(v for v in sorted({16 // elem_size, 4, 2, 1}, reverse=True) if fits(v))
