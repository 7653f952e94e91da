"""torch-facing wrappers of the C ABI (raw device pointers + current HIP stream).

PyTorch is plumbing here: device memory, streams, autograd glue.  All arithmetic of the
hot path happens in librlvi_gfx950.so; there is no eager/CPU fallback -- a missing library
or a non-GPU tensor raises.
"""
import ctypes

import torch

from . import _lib

_workspaces = {}


def _stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# the current stream's handle without building a torch.cuda.Stream object (MStepLoop asks once per batch)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (
    lambda dev: torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.RlviError(
                "rlvi_amd runs only on an MI355X HIP device: got a CPU tensor "
                "(there is no CPU fallback; the CPU restatement under oracle/ is test-only)")


class Workspace:
    """Caller-owned scratch + control words (include/rlvi_hip.h, 'Conventions')."""

    def __init__(self, device, max_n, max_b):
        L = _lib.load()
        self.max_n, self.max_b = int(max_n), int(max_b)
        self.nbytes = int(L.rlvi_workspace_bytes(self.max_n, self.max_b))
        self.buf = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 256 == 0
        # a sharded call that timed out leaves the ranks' round counters / warm-start state out of step:
        # further sharded calls are refused until rlvi_amd.dist.setup_peers(ws) has run again (all ranks)
        self.peers_stale = False
        _lib.check(L.rlvi_workspace_init(_ptr(self.buf), self.nbytes, _stream_ptr()),
                   "rlvi_workspace_init")

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr())

    def status(self):
        s = ctypes.c_int32(0)
        _lib.check(_lib.load().rlvi_workspace_status(self.ptr, ctypes.byref(s), _stream_ptr()),
                   "rlvi_workspace_status")
        return s.value

    def clear_status(self):
        _lib.check(_lib.load().rlvi_workspace_clear_status(self.ptr, _stream_ptr()),
                   "rlvi_workspace_clear_status")

    def set_option(self, name, value):
        """Per-workspace launch option (include/rlvi_hip.h, rlvi_workspace_set_option): "logits_from_hbm",
        "cold_start".  Host side, from the next launch on this workspace on."""
        _lib.check(_lib.load().rlvi_workspace_set_option(self.ptr, name.encode(), int(value)),
                   f"rlvi_workspace_set_option({name})")

    def reset_warm(self):
        """Forget the guesses the last E-step / threshold left for the next one."""
        _lib.check(_lib.load().rlvi_workspace_reset_warm(self.ptr, _stream_ptr()), "rlvi_workspace_reset_warm")

    def region(self, name):
        """(offset, bytes) of a named region of the layout ("records", "records_out", "warm", "scratch")."""
        n = ctypes.c_size_t(0)
        off = int(_lib.load().rlvi_workspace_region(name.encode(), ctypes.byref(n)))
        if off == ctypes.c_size_t(-1).value:
            raise ValueError(f"unknown workspace region {name!r}")
        return off, int(n.value)

    def pending_records(self):
        """True if accumulate-mode M-step records are waiting for an epoch_end / mstep_reduce (synchronises)."""
        off, n = self.region("records")
        return bool(self.buf[off:off + n].view(torch.float64).ne(0).any().item())

    def raise_on_status(self, what, mask=_lib.ST_RANGE | _lib.ST_TIMEOUT | _lib.ST_NOCONV):
        """Read the sticky device status (one 4-byte copy + stream sync) and raise RlviError on any
        flag of `mask`; the flag is cleared first so that the caller can recover and go on."""
        st = self.status()
        if st & mask:
            self.clear_status()
            if st & _lib.ST_TIMEOUT:
                self.peers_stale = True
            raise _lib.RlviError(f"{what}: device status {st}: {_lib.status_message(st & mask)}")
        return st


def debug_scratch_offset():
    """Byte offset of the workspace scratch area: the base of the slot table in which a stamps build run with
    RLVI_TJ_DEBUG=1 / RLVI_THR_DEBUG=1 leaves its stamps (rlvi_amd/csrc/rlvi_stamps.h, tools/stamps.py)."""
    return int(_lib.load().rlvi_workspace_region(b"scratch", None))


def workspace(device, n=0, b=0):
    """Per (device, stream) workspace, grown on demand."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream().cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.max_n < n or ws.max_b < b:
        ws = Workspace(device, max(n, ws.max_n if ws else 0, 1 << 16),
                       max(b, ws.max_b if ws else 0, 1 << 16))
        _workspaces[key] = ws
    return ws


# logit dtypes with C entries of their own, and the entries' name suffixes
_SUFFIX = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
_NATIVE = tuple(_SUFFIX)


def _entry(L, stem, dtype):
    """The C entry rlvi_<stem>_<f32 | bf16 | f16> for logits of a native dtype."""
    return getattr(L, f"rlvi_{stem}_{_SUFFIX[dtype]}")


def _as_logits(logits):
    """Logits as the C entries take them: a native dtype (any other goes to fp32), unit column stride."""
    if logits.dtype not in _NATIVE:
        logits = logits.float()
    return logits if logits.stride(1) == 1 else logits.contiguous()


def _as_int64(t):
    """Labels or sample indexes as a contiguous int64 vector."""
    return t if t.dtype == torch.int64 and t.is_contiguous() else t.to(torch.int64).contiguous()


def _check_f32_vectors(what, *tensors):
    """Vectors that a kernel reads or writes in place: each must be a contiguous 1-D fp32 tensor."""
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 1:
            raise ValueError(f"{what} must be contiguous 1-D fp32 tensors")


def _check_grad_scale(t, device, what="grad_scale"):
    """A one-element fp32 tensor on the logits' device that the kernel reads there (a GradScaler's scale, an upstream
    gradient), or None."""
    if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != 1 or t.device != device):
        raise ValueError(f"{what} must be a one-element fp32 tensor on the logits' device")
    return t


def _mstep_call(L, logits, labels, idx, weights, residuals, N, B, C, inv_scale, grad_scale, grad, out, ws):
    """The dtype's C entry.  fp16 reads the loss scale on the device (one rounding of the scaled gradient); fp32 and
    bf16 have no such argument: their gradient is multiplied by the scale tensor afterwards (stock AMP semantics)."""
    args = (_ptr(logits), logits.stride(0), _ptr(labels), _ptr(idx), _ptr(weights), _ptr(residuals), N, B, C,
            float(inv_scale))
    tail = (_ptr(grad), grad.stride(0) if grad is not None else 0, _ptr(out), ws.ptr, _stream_ptr())
    fn = _entry(L, "mstep_fwd_bwd", logits.dtype)
    if logits.dtype == torch.float16:
        return fn(*args, _ptr(grad_scale), *tail)
    rc = fn(*args, *tail)
    if rc == 0 and grad is not None and grad_scale is not None:
        grad.mul_(grad_scale)
    return rc


def mstep_fwd_bwd(logits, labels, idx, weights, residuals, inv_scale=None, want_grad=True,
                  out=None, grad=None, ws=None, accumulate=False, grad_scale=None):
    """One mini-batch of the M-step (train_rlvi.py:85-96 without model/optimizer).

    Scatters the per-sample NLL into `residuals[idx]`, gathers the lagged pi from
    `weights[idx]`, returns (out, grad) with out = fp32[4] device tensor
    {weighted mean loss, top-1 %, sum pi*l, hits} and grad = dL/dlogits (or None).
    accumulate=True: ONE launch, no scalars now (out is None): the per-batch sums pile up in the
    workspace until `epoch_end` / `mstep_reduce` collects them.
    fp32, bf16 and fp16 logits run natively; the gradient has the logits' dtype.  grad_scale: an optional
    one-element fp32 device tensor (a GradScaler's scale) that multiplies the gradient only -- read by the kernel
    for fp16 logits, no host sync either way.
    grad / out: optional buffers of the caller's.  grad must be [B, C] in the dtype the kernel runs the logits in, on
    their device, with unit column stride (rows may be strided); out four contiguous fp32 elements there: ValueError
    otherwise, before any launch.  The kernel's vector width follows the alignment of both blocks (include/rlvi_hip.h).
    """
    L = _lib.load()
    _require_gpu(logits, labels, idx, weights, residuals)
    if logits.dim() != 2:
        raise ValueError("logits must be [B, C]")
    B, C = logits.shape
    logits, labels = _as_logits(logits), _as_int64(labels)
    if idx is not None:
        idx = _as_int64(idx)
    if weights.dtype != torch.float32 or not weights.is_contiguous():
        raise ValueError("weights must be a contiguous fp32 vector (it is read in place)")
    if residuals is not None and (residuals.dtype != torch.float32 or not residuals.is_contiguous()):
        raise ValueError("residuals must be a contiguous fp32 vector (it is written in place)")
    N = weights.shape[0]
    if accumulate:
        out = None
    elif out is None:
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.float32 or out.numel() != 4 or not out.is_contiguous()
          or out.device != logits.device):
        raise ValueError("out must be four contiguous fp32 elements on the logits' device")
    if not want_grad:
        grad = None
    elif grad is None:
        grad = torch.empty((B, C), dtype=logits.dtype, device=logits.device)
    elif (not torch.is_tensor(grad) or grad.dim() != 2 or grad.shape != (B, C) or grad.dtype != logits.dtype
          or grad.device != logits.device or grad.stride(1) != 1):
        # (the C entry writes B rows of C elements of the logits' type at a pitch of grad.stride(0): anything else is
        #  garbage or a write out of bounds)
        raise ValueError(f"grad must be a [{B}, {C}] {logits.dtype} tensor on the logits' device with unit column "
                         "stride (rows may be strided)")
    grad_scale = _check_grad_scale(grad_scale, logits.device)
    ws = ws or workspace(logits.device, N, B)
    rc = _mstep_call(L, logits, labels, idx, weights, residuals, N, B, C,
                     inv_scale if inv_scale is not None else 1.0 / B, grad_scale, grad, out, ws)
    _lib.check(rc, "rlvi_mstep_fwd_bwd")
    return out, grad


def hint_logits_from_hbm(ws, flag=True):
    """Tell the M-step launcher where the logits of the calls ON THIS WORKSPACE come from.

    True: the [B, C] block streams from HBM -- it is larger than the Infinity Cache, or one of many blocks
    touched in rotation.  A one-tile-per-wave launch of 12 MB and more then holds its gradient stores until its
    reads have had their time at the HBM read rate (reads first, then writes, chip-wide: mstep.hip).  False (the
    default): nothing is assumed -- a chip-filling launch separates its reads from its writes per CU with a
    barrier behind the issue of its loads; the timed hold would cost time on a block that the model's last
    layer has just written and the cache serves (9.4 -> 10.3 us), which is what train_rlvi sees.
    Per workspace (round 3 had a process-wide knob): two loops on two streams do not see each other's hint."""
    ws.set_option("logits_from_hbm", 1 if flag else 0)


class MStepLoop:
    """mstep_fwd_bwd(..., accumulate=True) for a training loop, validated ONCE: the per-epoch vectors
    (weights, residuals), the workspace, the stream and the ctypes entry are fixed when the object is made
    (train_rlvi makes one per epoch), so a batch costs a handful of data_ptr() reads, one cached gradient
    buffer per batch shape and the foreign call -- the generic wrapper's ~10 checks, dict look-ups,
    c_void_p objects and current-stream query are what a 4-microsecond kernel at 4096 x 10 was waiting for.
    A batch that does not look like the validated form (strided logits or logits that are not fp32 / bf16 / fp16,
    labels or indexes that are not contiguous int64 device tensors, a loss scale that is not a one-element fp32
    tensor on the loop's device) takes the generic, fully checked path.

    grad_scale (optional): a GradScaler's scale tensor; the gradient comes back multiplied by it -- fp16 logits
    read it inside the kernel (one rounding, an overflow becomes inf), fp32 / bf16 multiply the buffer in place.
    The loss, the residuals and the epoch's records never see it.

    The returned gradient buffer is REUSED by the next batch of the same shape: consume it
    (`logits.backward(grad)`) before the next call, as train_rlvi does."""

    def __init__(self, weights, residuals, ws=None):
        L = _lib.load()
        _require_gpu(weights, residuals)
        _check_f32_vectors("weights / residuals", weights, residuals)
        if residuals.shape != weights.shape:
            raise ValueError("residuals and weights differ in length")
        self.weights, self.residuals = weights, residuals
        self.N = weights.shape[0]
        self.ws = ws or workspace(weights.device, self.N, 0)
        self._w, self._r, self._wsp = weights.data_ptr(), residuals.data_ptr(), self.ws.buf.data_ptr()
        self._stream = torch.cuda.current_stream(weights.device).cuda_stream
        self._f32, self._bf16, self._f16 = (_entry(L, "mstep_fwd_bwd", dt) for dt in _NATIVE)   # bound once
        self._grads = {}
        self._dev = weights.device
        self._devidx = weights.device.index if weights.device.index is not None else torch.cuda.current_device()

    def __call__(self, logits, labels, idx, inv_scale=None, grad_scale=None):
        dt = logits.dtype
        # the validated form, on the device and the stream the loop was made on; anything else -- strided or
        # other-typed logits, no index vector, a tensor on another device, a caller that has switched streams
        # inside the epoch -- takes the generic, fully checked wrapper (which launches on the CURRENT stream)
        if not (idx is not None and (dt is torch.float32 or dt is torch.bfloat16 or dt is torch.float16)
                and logits.dim() == 2
                and logits.is_contiguous() and labels.dtype is torch.int64 and idx.dtype is torch.int64
                and labels.is_contiguous() and idx.is_contiguous()
                and logits.device == self._dev and labels.is_cuda and idx.is_cuda
                and (grad_scale is None or (grad_scale.dtype is torch.float32 and grad_scale.numel() == 1
                                            and grad_scale.device == self._dev))
                and _raw_stream(self._devidx) == self._stream):
            _require_gpu(logits, labels, idx)
            _, grad = mstep_fwd_bwd(logits.detach(), labels, idx, self.weights, self.residuals,
                                    inv_scale=inv_scale, accumulate=True, ws=self.ws, grad_scale=grad_scale)
            return grad
        B, C = logits.shape
        key = (B, C, dt)
        grad = self._grads.get(key)
        if grad is None:
            grad = self._grads[key] = torch.empty((B, C), dtype=dt, device=self._dev)
        s = float(inv_scale) if inv_scale is not None else 1.0 / B
        if dt is torch.float16:
            rc = self._f16(logits.data_ptr(), C, labels.data_ptr(), idx.data_ptr(), self._w, self._r, self.N, B, C, s,
                           grad_scale.data_ptr() if grad_scale is not None else None, grad.data_ptr(), C, None,
                           self._wsp, self._stream)
        else:
            rc = (self._f32 if dt is torch.float32 else self._bf16)(
                logits.data_ptr(), C, labels.data_ptr(), idx.data_ptr(), self._w, self._r, self.N, B, C, s,
                grad.data_ptr(), C, None, self._wsp, self._stream)
            if grad_scale is not None and not rc:
                grad.mul_(grad_scale)
        if rc:
            _lib.check(rc, "rlvi_mstep_fwd_bwd")
        return grad


def estep_deep(residuals, weights, tol=1e-3, maxiter=40, iters=None, trace=None, ws=None):
    """update_sample_weights (train_rlvi.py:14-38), in place on both vectors."""
    L = _lib.load()
    _require_gpu(residuals, weights)
    _check_f32_vectors("residuals / weights", residuals, weights)
    if residuals.shape != weights.shape:
        raise ValueError("residuals and weights differ in length")
    N = weights.shape[0]
    ws = ws or workspace(weights.device, N, 0)
    rc = L.rlvi_estep_deep_f32(_ptr(residuals), _ptr(weights), N, float(tol), int(maxiter),
                               _ptr(iters), _ptr(trace), ws.ptr, _stream_ptr())
    _lib.check(rc, "rlvi_estep_deep_f32")


def evaluate_batch(logits, labels, out=None, ws=None):
    """Plain cross-entropy mean and top-1 percentage of one batch in one streaming pass over the
    logits (utils.evaluate, deep-learning/utils.py:48-62): out fp32[4] = {mean CE, top-1 %, sum
    CE, hits}."""
    L = _lib.load()
    _require_gpu(logits, labels)
    logits, labels = _as_logits(logits), _as_int64(labels)
    B, C = logits.shape
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
    ws = ws or workspace(logits.device, B, B)
    _lib.check(_mstep_call(L, logits, labels, None, None, None, B, B, C, 1.0 / B, None, None, out, ws),
               "rlvi_mstep_fwd_bwd (evaluation form)")
    return out


def mstep_reduce(scale=1.0, out=None, ws=None, device=None):
    """Collect (and clear) the records of accumulate-mode M-step calls -> out fp32[4]."""
    L = _lib.load()
    ws = ws or workspace(device or torch.cuda.current_device())
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=ws.buf.device)
    _lib.check(L.rlvi_mstep_reduce_f32(_ptr(out), float(scale), ws.ptr, _stream_ptr()),
               "rlvi_mstep_reduce_f32")
    return out


def _refuse_stale_peers(ws):
    if getattr(ws, "peers_stale", False):
        raise _lib.RlviError("a sharded call on this workspace timed out earlier: the ranks' round counters may "
                             "differ now -- run rlvi_amd.dist.setup_peers(ws) again on every rank first")


def estep_sharded(residuals, weights, n_all, tol=1e-3, maxiter=40, iters=None, ws=None, batches=0, out=None):
    """update_sample_weights (train_rlvi.py:14-38) with the samples sharded over the ranks: this rank's
    slice of residuals / weights in place, n_all samples over all ranks.  A collective over the ranks of
    the workspace's peer table (rlvi_amd.dist.setup_peers(ws) first).  Raises RlviError(RLVI_E_LIMIT)
    when the shape is outside the trajectory kernel.  batches > 0: `out` [4] also receives this rank's
    M-step scalars of the epoch (as epoch_end)."""
    L = _lib.load()
    _require_gpu(residuals, weights)
    _check_f32_vectors("residuals / weights", residuals, weights)
    if ws is None:
        raise ValueError("the sharded E-step needs the workspace whose peer table was set up")
    _refuse_stale_peers(ws)
    rc = L.rlvi_estep_sharded_f32(_ptr(residuals), _ptr(weights), weights.shape[0], int(n_all), float(tol),
                                  int(maxiter), int(batches), _ptr(out) if batches > 0 else None, _ptr(iters),
                                  ws.ptr, _stream_ptr())
    _lib.check(rc, "rlvi_estep_sharded_f32")


def threshold_truncate_sharded(weights, n_all, threshold, alpha=0.05, want_mask=False, ws=None):
    """threshold_truncate on weights sharded over the ranks (the companion of estep_sharded): the
    criterion over ALL ranks' weights, max(threshold, criterion), truncation of this rank's weights.
    Returns (threshold, mask of this rank's weights or None, kept over all ranks) -- rank-identical."""
    L = _lib.load()
    _require_gpu(weights)
    _check_f32_vectors("weights", weights)
    if ws is None:
        raise ValueError("the sharded threshold needs the workspace whose peer table was set up")
    _refuse_stale_peers(ws)
    thr = torch.as_tensor(threshold, dtype=torch.float32, device=weights.device).reshape(1).clone()
    mask = torch.empty(weights.shape[0], dtype=torch.uint8, device=weights.device) if want_mask else None
    kept = torch.zeros(1, dtype=torch.int64, device=weights.device)
    _lib.check(L.rlvi_threshold_truncate_sharded_f32(_ptr(weights), weights.shape[0], int(n_all), float(alpha),
                                                     _ptr(thr), _ptr(mask), _ptr(kept), ws.ptr, _stream_ptr()),
               "rlvi_threshold_truncate_sharded_f32")
    return thr.reshape(()), (mask.bool() if want_mask else None), kept.reshape(())


def epoch_end(residuals, weights, overfit=False, threshold=0, batches=0, tol=1e-3, maxiter=40,
              alpha=0.05, out=None, iters=None, ws=None):
    """train_rlvi.py:99-105 in one call: E-step over all samples, truncation when `overfit`, and
    the epoch's M-step scalars (out[1] = train_acc in percent when batches > 0).

    Returns (threshold, out): threshold is passed through unchanged while overfit is False, and
    a 0-dim device tensor after truncation ran; out is None when batches == 0."""
    L = _lib.load()
    _require_gpu(residuals, weights)
    _check_f32_vectors("residuals / weights", residuals, weights)
    N = weights.shape[0]
    ws = ws or workspace(weights.device, N, 0)
    thr = None
    if overfit:
        thr = torch.as_tensor(threshold, dtype=torch.float32, device=weights.device).reshape(1).clone()
    if batches > 0 and out is None:
        out = torch.empty(4, dtype=torch.float32, device=weights.device)
    rc = L.rlvi_epoch_end_f32(_ptr(residuals), _ptr(weights), N, float(tol), int(maxiter),
                              1 if overfit else 0, float(alpha), _ptr(thr), int(batches),
                              _ptr(out) if batches > 0 else None, _ptr(iters), ws.ptr,
                              _stream_ptr())
    _lib.check(rc, "rlvi_epoch_end_f32")
    return (thr.reshape(()) if overfit else threshold), (out if batches > 0 else None)


def fn_threshold(weights, alpha=0.05, ws=None):
    """false_negative_criterion (train_rlvi.py:41-49) -> 0-dim fp32 device tensor."""
    L = _lib.load()
    _require_gpu(weights)
    w = weights if (weights.dtype == torch.float32 and weights.is_contiguous()) \
        else weights.float().contiguous()
    thr = torch.empty(1, dtype=torch.float32, device=w.device)
    ws = ws or workspace(w.device, w.shape[0], 0)
    _lib.check(L.rlvi_fn_threshold_f32(_ptr(w), w.shape[0], float(alpha), _ptr(thr), ws.ptr,
                                       _stream_ptr()), "rlvi_fn_threshold_f32")
    return thr.reshape(())


def threshold_truncate(weights, threshold, alpha=0.05, want_mask=False, ws=None):
    """train_rlvi.py:102-103: threshold = max(threshold, criterion); weights[weights<thr] = 0.

    Returns (threshold 0-dim tensor, mask bool tensor or None, kept int64 0-dim tensor)."""
    L = _lib.load()
    _require_gpu(weights)
    if weights.dtype != torch.float32 or not weights.is_contiguous():
        raise ValueError("weights must be a contiguous fp32 vector (it is truncated in place)")
    N = weights.shape[0]
    thr = torch.as_tensor(threshold, dtype=torch.float32, device=weights.device).reshape(1).clone()
    mask = torch.empty(N, dtype=torch.uint8, device=weights.device) if want_mask else None
    kept = torch.zeros(1, dtype=torch.int64, device=weights.device)
    ws = ws or workspace(weights.device, N, 0)
    _lib.check(L.rlvi_threshold_truncate_f32(_ptr(weights), N, float(alpha), _ptr(thr), _ptr(mask),
                                             _ptr(kept), ws.ptr, _stream_ptr()),
               "rlvi_threshold_truncate_f32")
    return thr.reshape(()), (mask.bool() if want_mask else None), kept.reshape(())


def fused_em(logits, labels, pi, tol=1e-3, maxiter=40, inv_scale=None, want_grad=True, ws=None,
             out=None, grad=None, rows=None, iters=None):
    """In-batch E+M (online order): NLL -> E-step on this batch -> weighted loss + grad.

    `pi` [B] fp32 is read (first error only) and overwritten with the new posteriors.
    Returns (out[4], grad, loss_rows (min-shifted NLL), iters int32 tensor)."""
    L = _lib.load()
    _require_gpu(logits, labels, pi)
    if logits.dtype != torch.float32:
        logits = logits.float()
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    labels = _as_int64(labels)
    B, C = logits.shape
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
    if want_grad and grad is None:
        grad = torch.empty((B, C), dtype=torch.float32, device=logits.device)
    if not want_grad:
        grad = None
    if rows is None:
        rows = torch.empty(B, dtype=torch.float32, device=logits.device)
    if iters is None:
        iters = torch.zeros(1, dtype=torch.int32, device=logits.device)
    ws = ws or workspace(logits.device, B, B)
    rc = L.rlvi_fused_em_f32(_ptr(logits), logits.stride(0), _ptr(labels), _ptr(rows), _ptr(pi),
                             B, C, float(inv_scale if inv_scale is not None else 1.0 / B),
                             float(tol), int(maxiter), _ptr(grad),
                             grad.stride(0) if grad is not None else 0, _ptr(out), _ptr(iters),
                             ws.ptr, _stream_ptr())
    _lib.check(rc, "rlvi_fused_em_f32")
    return out, grad, rows, iters


def update_weights_f64(losses, tol=1e-3, maxiter=100, online=False):
    """standard-learning/rlvi.py:8-20 (online=False) or online-learning/main.py:45-58."""
    L = _lib.load()
    _require_gpu(losses)
    l = losses.to(torch.float64).contiguous()
    out = torch.empty_like(l)
    iters = torch.zeros(1, dtype=torch.int32, device=l.device)
    ws = workspace(l.device, l.shape[0], 0)
    fn = L.rlvi_update_weights_online_f64 if online else L.rlvi_update_weights_f64
    _lib.check(fn(_ptr(l), l.shape[0], float(tol), int(maxiter), _ptr(out), _ptr(iters), ws.ptr,
                  _stream_ptr()), "rlvi_update_weights_f64")
    return out, iters


def wls_solve(X, y, w, theta=None):
    """theta = argmin sum w_i (y_i - x_i.theta)^2 on the device (rlvi.py:70-71,:79-80): weighted Gram
    matrix on the fp64 MFMA units + Cholesky solve.  X [n, d <= 63] of full column rank."""
    L = _lib.load()
    _require_gpu(X, y, w)
    X = X.to(torch.float64).contiguous()
    n, d = X.shape
    if theta is None:
        theta = torch.empty(d, dtype=torch.float64, device=X.device)
    ws = workspace(X.device, n, 0)
    _lib.check(L.rlvi_wls_solve_f64(_ptr(X), _ptr(y.to(torch.float64).contiguous()),
                                    _ptr(w.to(torch.float64).contiguous()), n, d, _ptr(theta),
                                    ws.ptr, _stream_ptr()), "rlvi_wls_solve_f64")
    return theta


def linreg_losses(X, y, theta, w):
    """rlvi.py:72-74: losses = 0.5 (y - X theta)^2 / sigma2, sigma2 = w.r / sum(w)."""
    L = _lib.load()
    _require_gpu(X, y, theta, w)
    X = X.to(torch.float64).contiguous()
    n, d = X.shape
    losses = torch.empty(n, dtype=torch.float64, device=X.device)
    s2 = torch.empty(1, dtype=torch.float64, device=X.device)
    ws = workspace(X.device, n, 0)
    _lib.check(L.rlvi_linreg_losses_f64(_ptr(X), _ptr(y.to(torch.float64).contiguous()),
                                        _ptr(theta.to(torch.float64).contiguous()),
                                        _ptr(w.to(torch.float64).contiguous()), n, d,
                                        _ptr(losses), _ptr(s2), ws.ptr, _stream_ptr()),
               "rlvi_linreg_losses_f64")
    return losses, s2.reshape(())


def logistic_nll(X, w, b):
    """online-learning/main.py:295-296,:84-85: -log sigmoid(X w + b)."""
    L = _lib.load()
    _require_gpu(X, w)
    X = X.to(torch.float64).contiguous()
    n, d = X.shape
    losses = torch.empty(n, dtype=torch.float64, device=X.device)
    _lib.check(L.rlvi_logistic_nll_f64(_ptr(X), _ptr(w.to(torch.float64).contiguous()), float(b),
                                       n, d, _ptr(losses), _stream_ptr()),
               "rlvi_logistic_nll_f64")
    return losses


def linear_regression_check(n, d):
    """True if rlvi_linear_regression_f64 takes an [n, d] design in its one-launch form."""
    return _lib.load().rlvi_linear_regression_check(int(n), int(d)) == 0


def _fp64(t, dims=None, numel=None):
    """t is a contiguous fp64 tensor (of `dims` dimensions, of `numel` elements, where given)"""
    return (t.dtype == torch.float64 and t.is_contiguous() and (dims is None or t.dim() == dims)
            and (numel is None or t.numel() == numel))


def _one_launch(entry, inputs, args, outs, info, ws):
    """The call of a one-launch fp64 estimator on inputs its wrapper has checked:
    entry(*inputs, *inputs[0].shape, *args, *outs, info, ws, stream).  outs: one (tensor, elements) per output array;
    a tensor that is None is allocated here with that many elements -- or, with elements None as well, passed as
    NULL (an optional output).  info and the workspace are made when not given.  Returns (*outs, info).
    A batch entry: inputs[0] is [B, n, d], so that B travels in front of n, and info is int32[B, 4]."""
    L = _lib.load()
    X = inputs[0]
    batched = X.dim() == 3
    outs = [torch.empty(numel, dtype=torch.float64, device=X.device) if t is None and numel is not None else t
            for t, numel in outs]
    if info is None:
        info = torch.zeros((X.shape[0], 4) if batched else 4, dtype=torch.int32, device=X.device)
    ws = ws or workspace(X.device, X.shape[1 if batched else 0], 0)
    _lib.check(getattr(L, entry)(*[_ptr(t) for t in inputs], *X.shape, *args, *[_ptr(t) for t in outs], _ptr(info),
                                 ws.ptr, _stream_ptr()), entry)
    return (*outs, info)


def _design(what, bad, X, vectors, batched):
    """The input check of every estimator below: X is a contiguous fp64 device tensor [n, d] -- batched: [B, n, d] --
    and each of `vectors` one of its n (of its [B, n]) elements.  Returns (B, n, d), B = 1 unbatched.  `bad`: the
    single form's texts for an X that is not, and for a vector that is not."""
    _require_gpu(X, *vectors)
    if batched:
        if not _fp64(X, dims=3):
            raise ValueError(f"{what} [B, n, d] must be a contiguous fp64 device tensor")
        B, n, d = X.shape
        for v in vectors:
            if not (_fp64(v, dims=2) and v.shape[0] == B and v.shape[1] == n):
                raise ValueError(f"y must be a contiguous fp64 device tensor of {what}'s [B, n]")
        return B, n, d
    if not _fp64(X, dims=2):
        raise ValueError(bad[0])
    n, d = X.shape
    for v in vectors:
        if not _fp64(v, numel=n):
            raise ValueError(bad[1])
    return 1, n, d


def _theta_init(theta_init, d):
    """the pointer of pca's theta_init [d] (NULL for None), checked"""
    if theta_init is not None:
        _require_gpu(theta_init)
        if not _fp64(theta_init, numel=d):
            raise ValueError("theta_init must be a contiguous fp64 device tensor of d elements")
    return _ptr(theta_init)


class _Estimator:
    """A one-launch fp64 estimator with a batch form, written once for both: the stem of its C entries
    (rlvi_<stem>_f64 and rlvi_<stem>_batch_f64), scalars(n, d, *the wrapper's keyword values) -> the entry's scalar
    arguments, lengths(n, d) -> the elements of one problem's part of each output, optional: the last output is NULL
    unless given (where False, one that is not given is allocated), square: the first output is a [d, d] matrix, the
    design's name in messages and the single form's texts for a bad design and a bad vector.  The batch form is the
    single form with a leading B: outputs of B x length elements, results viewed [B, ...], info int32[B, 4]."""

    def __init__(self, stem, scalars, lengths, optional=False, square=False, what="X", bad=None):
        self.entries = (f"rlvi_{stem}_f64", f"rlvi_{stem}_batch_f64")
        self.scalars, self.lengths, self.optional, self.square, self.what = scalars, lengths, optional, square, what
        self.bad = bad or (f"{what} [n, d] must be a contiguous fp64 device tensor",
                           f"y and the weights must be contiguous fp64 device tensors of {what}'s n elements")

    def __call__(self, batched, inputs, values, outs, info, ws):
        """The single (batched False) or the batch form on the wrapper's inputs, keyword values and output tensors
        (None: allocated here) -> (first output, second output, info)."""
        B, n, d = _design(self.what, self.bad, inputs[0], inputs[1:], batched)
        lengths = self.lengths(n, d)
        if len(outs) != len(lengths):
            raise ValueError(f"{len(lengths)} output tensors (or None) are expected, not {len(outs)}")
        sized = [(t, B * k) for t, k in zip(outs, lengths)]
        if batched:
            for t, k in zip(outs, lengths):
                if t is not None:
                    _require_gpu(t)
                    if not _fp64(t, numel=B * k):
                        raise ValueError(f"an output must be a contiguous fp64 device tensor of {B} x {k} elements")
        if self.optional and outs[-1] is None:
            sized[-1] = (None, None)
        res = _one_launch(self.entries[batched], inputs, self.scalars(n, d, *values), sized, info, ws)
        first, second, info = res[0], res[1], res[-1]
        if batched:
            first, second, info = first.view(B, -1), second.view(B, -1), info.view(B, 4)
        if self.square:
            first = first.view(B, d, d) if batched else first.view(d, d)
        return first, second, info


def _theta_weights(n, d):
    return d, n


def _matrix_weights(n, d):
    return d * d, n


def _rlvi_scalars(n, d, maxiter, tol, estep_tol, estep_maxiter):
    return int(maxiter), float(tol), float(estep_tol), int(estep_maxiter)


def _rrm_scalars(n, d, eps, maxiter, tol):
    return float(eps), int(maxiter), float(tol)


_XY_BAD = ("X [n, d] and y [n] must be contiguous fp64 device tensors",) * 2
_LINREG = _Estimator("linear_regression", _rlvi_scalars, _theta_weights, bad=_XY_BAD)
_LOGREG = _Estimator("logistic_regression",
                     lambda n, d, maxiter, tol, estep_tol, estep_maxiter, C:
                     (int(maxiter), float(tol), float(estep_tol), int(estep_maxiter), float(C)),
                     lambda n, d: (d + 1, n, n), optional=True)          # (losses)
_MEAN = _Estimator("robust_mean", _rlvi_scalars, _theta_weights, what="sample")
_PCA = _Estimator("robust_pca",
                  lambda n, d, maxiter, tol, theta_init, estep_tol, estep_maxiter:
                  (int(maxiter), float(tol), _theta_init(theta_init, d), float(estep_tol), int(estep_maxiter)),
                  _theta_weights, what="sample")
_COVARIANCE = _Estimator("robust_covariance",
                         lambda n, d, n_eff, maxiter, tol, estep_tol, estep_maxiter:
                         (float(n_eff), int(maxiter), float(tol), float(estep_tol), int(estep_maxiter)),
                         _matrix_weights, square=True, what="sample")
_RRM_MEAN = _Estimator("rrm_mean", _rrm_scalars, _theta_weights, what="sample")
_RRM_PCA = _Estimator("rrm_pca",
                      lambda n, d, eps, maxiter, tol, theta_init:
                      (float(eps), int(maxiter), float(tol), _theta_init(theta_init, d)),
                      _theta_weights, what="sample")
_RRM_COVARIANCE = _Estimator("rrm_covariance", _rrm_scalars, _matrix_weights, square=True, what="sample")
_RRM_LINREG = _Estimator("rrm_linear_regression", _rrm_scalars, _theta_weights, bad=_XY_BAD)
_HUBER_LINREG = _Estimator("huber_linear_regression",
                           lambda n, d, c, sigma0, maxiter: (float(c), float(sigma0), int(maxiter)),
                           lambda n, d: (d, 1), bad=_XY_BAD)
_RRM_LOGREG = _Estimator("rrm_logistic_regression",
                         lambda n, d, eps, maxiter, tol, C: (float(eps), int(maxiter), float(tol), float(C)),
                         lambda n, d: (d + 1, n))
_NO_OUT = (None, None)


def linear_regression(X, y, maxiter=100, tol=1e-3, estep_tol=1e-3, estep_maxiter=100, theta=None, weights=None,
                      info=None, ws=None):
    """linear_regression(X, y, maxiter, tol) of standard-learning/rlvi.py:68-89 as ONE launch on device tensors
    (no host synchronisation here).  Returns (theta [d], weights [n], info int32[4] = {outer iterations, inner
    iterations of the last E-step, inner iterations in all, fallback}) -- info[3] == 1 (rank-deficient design):
    theta / weights were not written, compose wls_solve / linreg_losses / update_weights_f64 instead."""
    return _LINREG(False, (X, y), (maxiter, tol, estep_tol, estep_maxiter), (theta, weights), info, ws)


def logistic_regression_check(n, d):
    """True if rlvi_logistic_regression_f64 / rlvi_logistic_fit_f64 take an [n, d] design (n <= 4096, d <= 30)."""
    return _lib.load().rlvi_logistic_regression_check(int(n), int(d)) == 0


def logistic_fit(X, y, w, C=100.0, theta=None, losses=None, info=None, ws=None):
    """utils.sklearn_log_reg(X, y, weights) of standard-learning/utils.py:61-73 as ONE launch on device tensors
    (rlvi_logistic_fit_f64; no host synchronisation here): the minimiser of 1/2 v.v + C sum (w_i / max w)
    log(1 + exp(-s_i z_i)) that liblinear approximates, by Newton to the rounding floor.  Returns (theta [d + 1] =
    (intercept, coef), losses [n] = log(1 + exp(z)), info int32[4] = {0, 0, Newton steps, flag}); flag 1: nothing
    was written (data not finite, y not 0 / 1, no positive weight, a pivot not safely positive); flag 2: the Newton cap, or a line search
    without an acceptable step (RLVI_ST_NOCONV in ws)."""
    _, n, d = _design("X", _LOGREG.bad, X, (y, w), False)
    return _one_launch("rlvi_logistic_fit_f64", (X, y, w), (float(C),), ((theta, d + 1), (losses, n)), info, ws)


def logistic_regression(X, y, maxiter=100, tol=1e-2, estep_tol=1e-3, estep_maxiter=100, C=100.0, theta=None,
                        weights=None, losses=None, info=None, ws=None):
    """logistic_regression(X, y, maxiter, tol) of standard-learning/rlvi.py:92-108 as ONE launch on device tensors
    (rlvi_logistic_regression_f64; no host synchronisation here).  Returns (theta [d + 1] = (intercept, coef),
    weights [n], info int32[4] = {outer iterations, inner iterations of the last E-step, Newton steps in all, flag});
    `losses` [n], if given, receives the last fit's.  flag as logistic_fit."""
    return _LOGREG(False, (X, y), (maxiter, tol, estep_tol, estep_maxiter, C), (theta, weights, losses), info, ws)


def moments_check(n, d):
    """True if rlvi_robust_mean_f64 / _pca_f64 / _covariance_f64 take an [n, d] sample (2 <= n <= 4096, 1 <= d <= 8,
    n d <= 16 384: the sample is resident in LDS)."""
    return _lib.load().rlvi_moments_check(int(n), int(d)) == 0


def robust_mean(sample, maxiter=100, tol=1e-3, estep_tol=1e-3, estep_maxiter=100, theta=None, weights=None, info=None,
                ws=None):
    """mean(sample, maxiter, tol) of standard-learning/rlvi.py:46-65 as ONE launch on device tensors
    (rlvi_robust_mean_f64; no host synchronisation here).  Returns (theta [d], weights [n], info int32[4] = {outer
    iterations, inner iterations of the last E-step, inner iterations in all, flag}); flag 1: nothing was written
    (data not finite, a variance not safely positive)."""
    return _MEAN(False, (sample,), (maxiter, tol, estep_tol, estep_maxiter), (theta, weights), info, ws)


def robust_pca(sample, maxiter=100, tol=1e-2, theta_init=None, estep_tol=1e-3, estep_maxiter=100, theta=None,
               weights=None, info=None, ws=None):
    """pca(sample, maxiter, tol, theta_init) of standard-learning/rlvi.py:111-125 as ONE launch on device tensors
    (rlvi_robust_pca_f64).  theta_init [d] (fp64, on the device) replaces the first fit and is used as is.  Returns
    (theta [d], weights [n], info = {outer, inner of the last E-step, Jacobi sweeps in all, flag}); flag 2: an
    eigen-solve hit its 30 sweeps (RLVI_ST_NOCONV in ws)."""
    return _PCA(False, (sample,), (maxiter, tol, theta_init, estep_tol, estep_maxiter), (theta, weights), info, ws)


def robust_covariance(sample, n_eff, maxiter=100, tol=1e-2, estep_tol=1e-3, estep_maxiter=100, theta=None,
                      weights=None, info=None, ws=None):
    """covariance(sample, eps, maxiter, tol) of standard-learning/rlvi.py:128-144 with n_eff = n (1 - eps) as ONE
    launch on device tensors (rlvi_robust_covariance_f64).  Returns (theta [d, d], weights [n], info = {outer, inner
    of the last E-step, E-steps with the constraint active, flag}); flag 1: nothing was written (data not finite, a
    pivot not safely positive, n_eff outside (0, n)); flag 2: a root-find hit its cap (RLVI_ST_NOCONV in ws)."""
    return _COVARIANCE(False, (sample,), (n_eff, maxiter, tol, estep_tol, estep_maxiter), (theta, weights), info, ws)


# ---- a Monte-Carlo sweep in ONE launch: B problems of one shape, one workgroup each.  The single forms' keywords; the
# arrays carry a leading batch dimension; problem b gets the bits of the single call on it alone.
def linear_regression_batch(X, y, maxiter=100, tol=1e-3, estep_tol=1e-3, estep_maxiter=100, theta=None,
                            weights=None, info=None, ws=None):
    """B linear regressions (linear_regression above; the loop of standard-learning/main.py:261-273) as ONE launch
    (rlvi_linear_regression_batch_f64): X [B, n, d], y [B, n] -> (theta [B, d], weights [B, n], info int32[B, 4]).
    info[b, 3] == 1: problem b is rank-deficient, its rows were not written -- the general path is the caller's."""
    return _LINREG(True, (X, y), (maxiter, tol, estep_tol, estep_maxiter), (theta, weights), info, ws)


def logistic_regression_batch(X, y, maxiter=100, tol=1e-2, estep_tol=1e-3, estep_maxiter=100, C=100.0, theta=None,
                              weights=None, losses=None, info=None, ws=None):
    """B logistic regressions (logistic_regression above; main.py:431-437) as ONE launch
    (rlvi_logistic_regression_batch_f64): X [B, n, d], y [B, n] -> (theta [B, d + 1], weights [B, n], info
    int32[B, 4]); `losses` [B, n], if given, receives the last fits'."""
    return _LOGREG(True, (X, y), (maxiter, tol, estep_tol, estep_maxiter, C), (theta, weights, losses), info, ws)


def robust_mean_batch(sample, maxiter=100, tol=1e-3, estep_tol=1e-3, estep_maxiter=100, theta=None, weights=None,
                      info=None, ws=None):
    """B robust means (robust_mean above; main.py:180-188) as ONE launch (rlvi_robust_mean_batch_f64): sample
    [B, n, d] -> (theta [B, d], weights [B, n], info int32[B, 4])."""
    return _MEAN(True, (sample,), (maxiter, tol, estep_tol, estep_maxiter), (theta, weights), info, ws)


def robust_pca_batch(sample, maxiter=100, tol=1e-2, theta_init=None, estep_tol=1e-3, estep_maxiter=100, theta=None,
                     weights=None, info=None, ws=None):
    """B robust PCAs (robust_pca above; main.py:489-494) as ONE launch (rlvi_robust_pca_batch_f64): sample [B, n, d],
    theta_init [d] for all of them (or None) -> (theta [B, d], weights [B, n], info int32[B, 4])."""
    return _PCA(True, (sample,), (maxiter, tol, theta_init, estep_tol, estep_maxiter), (theta, weights), info, ws)


def robust_covariance_batch(sample, n_eff, maxiter=100, tol=1e-2, estep_tol=1e-3, estep_maxiter=100, theta=None,
                            weights=None, info=None, ws=None):
    """B robust covariances (robust_covariance above; main.py:539-544) as ONE launch
    (rlvi_robust_covariance_batch_f64): sample [B, n, d], one n_eff = n (1 - eps) for all of them -> (theta
    [B, d, d], weights [B, n], info int32[B, 4])."""
    return _COVARIANCE(True, (sample,), (n_eff, maxiter, tol, estep_tol, estep_maxiter), (theta, weights), info, ws)


def update_weights_constrained(losses, n_eff, tol=1e-3, maxiter=100, out=None, info=None, ws=None):
    """update_weights_constrained(losses, n_eff, tol, maxiter) of standard-learning/rlvi.py:23-43 as ONE launch on a
    device tensor of n <= 4096 losses (rlvi_update_weights_constrained_f64): the plain fixed point, then, if its
    weights sum to less than n_eff, the weights 1 / (1 + c exp(l - s)) at the exact root s of their sum = n_eff.
    Returns (weights [n], info int32[4] = {root-find evaluations, the fixed point's iterations, 1 if the constraint
    was active, flag})."""
    _require_gpu(losses)
    if not _fp64(losses, dims=1):
        raise ValueError("losses [n] must be a contiguous fp64 device tensor")
    return _one_launch("rlvi_update_weights_constrained_f64", (losses,), (float(n_eff), float(tol), int(maxiter)),
                       ((out, losses.shape[0]),), info, ws)


# ---- Robust Risk Minimization (standard-learning/rrm.py): the same kernels with the RRM weight rule; eps where the
# entries above take n_eff, info = {outer, evaluations of the last root-find, evaluations | Jacobi sweeps in all, flag}.
def rrm_mean(sample, eps, maxiter=100, tol=1e-3, theta=None, weights=None, info=None, ws=None):
    """mean(sample, eps, maxiter, tol) of standard-learning/rrm.py:36-52 as ONE launch on device tensors
    (rlvi_rrm_mean_f64; no host synchronisation here).  Returns (theta [d], weights [n], info int32[4]); flag 1:
    nothing was written (data or a loss not finite, eps outside (0, 1), (1 - eps) n <= 1); flag 2: a root-find hit its
    200 evaluations (RLVI_ST_NOCONV in ws)."""
    return _RRM_MEAN(False, (sample,), (eps, maxiter, tol), (theta, weights), info, ws)


def rrm_pca(sample, eps, maxiter=100, tol=1e-2, theta_init=None, theta=None, weights=None, info=None, ws=None):
    """pca(sample, eps, maxiter, tol, theta_init) of standard-learning/rrm.py:94-107 as ONE launch on device tensors
    (rlvi_rrm_pca_f64); theta_init as for robust_pca.  Returns (theta [d], weights [n], info); info[2]: Jacobi sweeps
    in all."""
    return _RRM_PCA(False, (sample,), (eps, maxiter, tol, theta_init), (theta, weights), info, ws)


def rrm_covariance(sample, eps, maxiter=100, tol=1e-2, theta=None, weights=None, info=None, ws=None):
    """covariance(sample, eps, maxiter, tol) of standard-learning/rrm.py:110-124 as ONE launch on device tensors
    (rlvi_rrm_covariance_f64).  Returns (theta [d, d], weights [n], info); flag 1 as for rrm_mean, and a pivot that
    is not safely positive."""
    return _RRM_COVARIANCE(False, (sample,), (eps, maxiter, tol), (theta, weights), info, ws)


def rrm_mean_batch(sample, eps, maxiter=100, tol=1e-3, theta=None, weights=None, info=None, ws=None):
    """B calls of rrm_mean (the rrm.mean of main.py:180-188) as ONE launch (rlvi_rrm_mean_batch_f64): sample
    [B, n, d], one eps for all -> (theta [B, d], weights [B, n], info int32[B, 4])."""
    return _RRM_MEAN(True, (sample,), (eps, maxiter, tol), (theta, weights), info, ws)


def rrm_pca_batch(sample, eps, maxiter=100, tol=1e-2, theta_init=None, theta=None, weights=None, info=None, ws=None):
    """B calls of rrm_pca (main.py:489-494) as ONE launch (rlvi_rrm_pca_batch_f64): sample [B, n, d], one eps and one
    theta_init [d] (or None) for all -> (theta [B, d], weights [B, n], info int32[B, 4])."""
    return _RRM_PCA(True, (sample,), (eps, maxiter, tol, theta_init), (theta, weights), info, ws)


def rrm_covariance_batch(sample, eps, maxiter=100, tol=1e-2, theta=None, weights=None, info=None, ws=None):
    """B calls of rrm_covariance (main.py:539-544) as ONE launch (rlvi_rrm_covariance_batch_f64): sample [B, n, d],
    one eps for all -> (theta [B, d, d], weights [B, n], info int32[B, 4])."""
    return _RRM_COVARIANCE(True, (sample,), (eps, maxiter, tol), (theta, weights), info, ws)


def rrm_update_weights(losses, eps, out=None, info=None, ws=None):
    """update_weights(losses, eps) of standard-learning/rrm.py:12-33 as ONE launch on a device tensor of n <= 4096
    losses (rlvi_rrm_update_weights_f64): exp(-l / alpha) / sum exp(-l / alpha) at the alpha where their entropy is
    log((1 - eps) n) -- the exact root of what the reference minimises by Brent's search; with no root, 1 / m on the m
    minima.  Returns (weights [n], info int32[4] = {evaluations, 0, 1 if there was a root, flag})."""
    _require_gpu(losses)
    if not _fp64(losses, dims=1):
        raise ValueError("losses [n] must be a contiguous fp64 device tensor")
    return _one_launch("rlvi_rrm_update_weights_f64", (losses,), (float(eps),), ((out, losses.shape[0]),), info, ws)


# ---- the robust linear regressions of standard-learning/main.py:248-357 (robust_linreg.hip)
def rrm_linear_regression(X, y, eps, maxiter=100, tol=1e-3, out=None, info=None, ws=None):
    """linear_regression(X, y, eps, maxiter, tol) of standard-learning/rrm.py:55-73 as ONE launch on device tensors
    (rlvi_rrm_linear_regression_f64; no host synchronisation here).  out: (theta [d], weights [n]) to write into, or
    None.  Returns (theta, weights, info int32[4] = {outer iterations, evaluations of the last root-find, evaluations in
    all, flag}); flag 1 (a pivot not safely positive: compose rrm_update_weights / wls_solve instead) and flag 2 (a
    loss not finite): nothing was written; flag 3: a root-find hit its 200 evaluations (RLVI_ST_NOCONV in ws)."""
    return _RRM_LINREG(False, (X, y), (eps, maxiter, tol), out or _NO_OUT, info, ws)


def rrm_linear_regression_batch(X, y, eps, maxiter=100, tol=1e-3, out=None, info=None, ws=None):
    """B calls of rrm_linear_regression (the sweep of main.py:261-273) as ONE launch
    (rlvi_rrm_linear_regression_batch_f64): X [B, n, d], y [B, n], one eps for all -> (theta [B, d], weights [B, n],
    info int32[B, 4]); problem b has the bits of its single call."""
    return _RRM_LINREG(True, (X, y), (eps, maxiter, tol), out or _NO_OUT, info, ws)


def huber_linear_regression(X, y, c=0.7317, sigma0=1.0, maxiter=1000, out=None, info=None, ws=None):
    """linear_regression(X, y, c, sigma0) of standard-learning/huber.py:13-40 as ONE launch on device tensors
    (rlvi_huber_linear_regression_f64; no host synchronisation here); the reference's `while True` is capped at
    maxiter.  out: (theta [d], scale [1]) to write into, or None.  Returns (theta, scale -- the last sigma --, info
    int32[4] = {iterations, 0, 0, flag}); flag 1 (X^T X singular) and flag 2 (a scale not positive and finite, a theta
    not finite): nothing was written; flag 3: the cap was reached while the iteration still moved (RLVI_ST_NOCONV in
    ws, the last iterate written)."""
    return _HUBER_LINREG(False, (X, y), (c, sigma0, maxiter), out or _NO_OUT, info, ws)


def huber_linear_regression_batch(X, y, c=0.7317, sigma0=1.0, maxiter=1000, out=None, info=None, ws=None):
    """B calls of huber_linear_regression (the sweep of main.py:261-273) as ONE launch
    (rlvi_huber_linear_regression_batch_f64): X [B, n, d], y [B, n], one c and sigma0 for all -> (theta [B, d], scale
    [B], info int32[B, 4]); problem b has the bits of its single call."""
    theta, scale, info = _HUBER_LINREG(True, (X, y), (c, sigma0, maxiter), out or _NO_OUT, info, ws)
    return theta, scale.view(-1), info


# ---- RRM's logistic regression of standard-learning/main.py:361-470 (robust_logreg.hip)
def rrm_logistic_regression(X, y, eps, maxiter=100, tol=1e-2, C=100.0, out=None, info=None, ws=None):
    """logistic_regression(X, y, eps, maxiter, tol) of standard-learning/rrm.py:76-91 as ONE launch on device tensors
    (rlvi_rrm_logistic_regression_f64; no host synchronisation here).  out: (theta [d + 1], weights [n]) to write
    into, or None.  Returns (theta = (intercept, coef), weights, info int32[4] = {outer iterations, evaluations of the
    last root-find, Newton steps in all, flag}); flag 1 (a label not 0 / 1, a value not finite): nothing was written;
    flag 2 (a fit at its Newton cap or without an acceptable step) and flag 3 (a root-find at its 200 evaluations):
    RLVI_ST_NOCONV in ws, the results written."""
    return _RRM_LOGREG(False, (X, y), (eps, maxiter, tol, C), out or _NO_OUT, info, ws)


def rrm_logistic_regression_batch(X, y, eps, maxiter=100, tol=1e-2, C=100.0, out=None, info=None, ws=None):
    """B calls of rrm_logistic_regression (the sweep of main.py:372-401) as ONE launch
    (rlvi_rrm_logistic_regression_batch_f64): X [B, n, d], y [B, n], one eps for all -> (theta [B, d + 1], weights
    [B, n], info int32[B, 4]); problem b has the bits of its single call."""
    return _RRM_LOGREG(True, (X, y), (eps, maxiter, tol, C), out or _NO_OUT, info, ws)


def sample_weight_online(X, coef, intercept=0.0, first=False, tol=1e-3, maxiter=100, out=None, losses=None,
                         iters=None):
    """One mini-batch of online-learning/main.py:293-297 in ONE launch on device tensors: residuals =
    -log sigmoid(X coef + intercept) (log 2 for the first batch), sample_weight = update_weights_rlvi(residuals).
    Returns (sample_weight [n], losses or None, iters or None)."""
    L = _lib.load()
    _require_gpu(X, coef)
    n, d = X.shape
    if not first and (X.dtype != torch.float64 or not X.is_contiguous() or coef.dtype != torch.float64):
        raise ValueError("X [n, d] and coef [d] must be contiguous fp64 device tensors")
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=X.device)
    _lib.check(L.rlvi_sample_weight_online_f64(_ptr(X), _ptr(coef), float(intercept), 1 if first else 0, n, d,
                                               float(tol), int(maxiter), _ptr(losses), _ptr(out), _ptr(iters),
                                               _stream_ptr()), "rlvi_sample_weight_online_f64")
    return out, losses, iters


# ---- the online path's mini-batch and stream (online_sgd.hip)
ONLINE_METHODS = {"SGD": 0, "RLVI": 1, "RRM": 2, "GIVEN": 3}
# info[..., 3] of online_step / online_stream -> (exception class -- None: RlviError --, text); read by
# rlvi_amd.online._raise_flags
ONLINE_FLAGS = {
    1: (ValueError, "Floating-point under-/overflow occurred at epoch #1. Scaling input data with StandardScaler or "
                    "MinMaxScaler might help."),
    2: (ValueError, "{name}: no sample weights -- a residual is not finite, or (1 - eps) n <= 1"),
    3: (None, "{name}: RRM's root-find did not end within its 200 evaluations"),
    4: (ValueError, "{name}: an index of the order, or a row count, is out of range"),
}


class _Online:
    """The two entries of online_sgd.hip, written once: what a design, a label vector, the test rows, an order and an
    output must be -- `lead` the leading dimensions ((), or (T,) for the stream) --, and the allocation of the outputs
    that are not given."""

    def __init__(self, entry):
        self.entry = entry

    @staticmethod
    def _f64(t, shape, what):
        if t is None or not (_fp64(t) and tuple(t.shape) == tuple(shape)):
            raise ValueError(f"{what} must be a contiguous fp64 device tensor of shape {list(shape)}")
        return t

    @staticmethod
    def _i32(t, shape, what, device, optional=True, zero=False):
        if t is None:
            if optional:
                return None
            return (torch.zeros if zero else torch.empty)(shape, dtype=torch.int32, device=device)
        if not (t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)
                and t.device == device):
            raise ValueError(f"{what} must be a contiguous int32 device tensor of shape {list(shape)}")
        return t

    def inputs(self, X, y, X_test, y_test, lead):
        """(n, d, m) of checked inputs; the test rows may both be None (m = 0)"""
        if (X_test is None) != (y_test is None):
            raise ValueError("X_test and y_test come together")
        _require_gpu(*[t for t in (X, y, X_test, y_test) if t is not None])
        k = len(lead)
        if not (torch.is_tensor(X) and X.dim() == k + 2 and tuple(X.shape[:k]) == tuple(lead)):
            raise ValueError(f"X must be a contiguous fp64 device tensor of shape {[*lead, 'n', 'd']}")
        n, d = X.shape[k:]
        self._f64(X, (*lead, n, d), "X")
        self._f64(y, (*lead, n), "y")
        m = 0
        if X_test is not None:
            if X_test.dim() != k + 2:
                raise ValueError(f"X_test must be a contiguous fp64 device tensor of shape {[*lead, 'm', d]}")
            m = X_test.shape[k]
            self._f64(X_test, (*lead, m, d), "X_test")
            self._f64(y_test, (*lead, m), "y_test")
        return n, d, m


_ONLINE_STEP = _Online("rlvi_online_step_f64")
_ONLINE_STREAM = _Online("rlvi_online_stream_f64")


def _online_method(m):
    if isinstance(m, str):
        if m not in ONLINE_METHODS:
            raise ValueError(f"method must be one of {sorted(ONLINE_METHODS)} or 0 .. 3, not {m!r}")
        return ONLINE_METHODS[m]
    return int(m)


def online_step(X, y, state, method="SGD", eps=0.3, first=False, order=None, X_test=None, y_test=None, alpha=1e-4,
                tol=1e-3, maxiter=100, sample_weight=None, counts=None, info=None):
    """One mini-batch of online-learning/main.py:291-313, :318-331 for one classifier in ONE launch on device tensors
    (rlvi_online_step_f64; no host synchronisation here): residuals -> sample weights (method 'SGD': ones, 'RLVI':
    update_weights_rlvi, 'RRM': update_weights_rrm(eps), 'GIVEN': sample_weight as passed) -> one partial_fit pass of
    scikit-learn's SGDClassifier(loss='log_loss', random_state=1, alpha=alpha) over the rows in `order` (int32 [n],
    rlvi_amd.online.sgd_order(n); None: natural order) -> the counts (tp, tn, fp, fn) of the test rows under the new
    state.  state [d + 2] = (coef, intercept, t) is updated in place (first: the unfitted classifier, whatever state
    holds).  Returns (state, sample_weight [n], counts int32[4], info int32[4] = {E-step iterations or root-find
    evaluations, 1 if RRM had a root, samples with a non-zero update, flag}); the flags are ONLINE_FLAGS."""
    L = _lib.load()
    n, d, m = _ONLINE_STEP.inputs(X, y, X_test, y_test, ())
    _require_gpu(state)
    _Online._f64(state, (d + 2,), "state")
    method = _online_method(method)
    dev = X.device
    if sample_weight is None:
        if method == 3:
            raise ValueError("method 'GIVEN' needs sample_weight")
        sample_weight = torch.empty(n, dtype=torch.float64, device=dev)
    _require_gpu(sample_weight)
    _Online._f64(sample_weight, (n,), "sample_weight")
    order = _Online._i32(order, (n,), "order", dev)
    counts = _Online._i32(counts, (4,), "counts", dev, optional=False)
    info = _Online._i32(info, (4,), "info", dev, optional=False, zero=True)
    _lib.check(L.rlvi_online_step_f64(_ptr(X), _ptr(y), _ptr(order), n, d, method, float(eps), 1 if first else 0,
                                      _ptr(state), _ptr(X_test), _ptr(y_test), m, float(alpha), float(tol),
                                      int(maxiter), _ptr(sample_weight), _ptr(counts), _ptr(info), _stream_ptr()),
               "rlvi_online_step_f64")
    return state, sample_weight, counts, info


def online_stream(X, y, X_test, y_test, methods=("SGD", "RRM", "RLVI"), eps=0.3, rows=None, orders=None, alpha=1e-4,
                  tol=1e-3, maxiter=100, weights=None, want_weights=True, state_hist=None, counts=None, info=None):
    """The loop of online-learning/main.py:288-339 -- T consecutive mini-batches for S <= 8 classifiers -- in ONE launch
    (rlvi_online_stream_f64), one workgroup per classifier, every classifier unfitted at the start.  X [T, n, d], y
    [T, n], X_test [T, m, d], y_test [T, m] padded to the largest batch (the test rows may be None); rows int32 [T, 2] =
    (n_t, m_t), the real row counts (None: all of them); orders int32 [T, n] (None: natural order).  eps: one value, or
    one per classifier.  weights [S, T, n]: written by the methods that compute theirs, read by a 'GIVEN' (which needs
    it); without it the weights are kept (want_weights) or not.  Returns (state_hist [S, T, d + 2], counts int32[S, T, 4],
    weights or None, info int32[S, T, 4]); (classifier s, batch t) has the bits of the same sequence of online_step."""
    L = _lib.load()
    if not (torch.is_tensor(X) and X.dim() == 3):
        raise ValueError("X must be a contiguous fp64 device tensor of shape ['T', 'n', 'd']")
    T = X.shape[0]
    n, d, m = _ONLINE_STREAM.inputs(X, y, X_test, y_test, (T,))
    codes = [_online_method(v) for v in methods]
    S = len(codes)
    if not 1 <= S <= 8:
        raise ValueError("1 to 8 methods are expected")
    eps = [float(eps)] * S if isinstance(eps, (int, float)) else [float(e) for e in eps]
    if len(eps) != S:
        raise ValueError("eps: one value, or one per method")
    dev = X.device
    if weights is None and (want_weights or 3 in codes):
        if 3 in codes:
            raise ValueError("method 'GIVEN' needs weights [S, T, n]")
        weights = torch.zeros((S, T, n), dtype=torch.float64, device=dev)
    if weights is not None:
        _require_gpu(weights)
        _Online._f64(weights, (S, T, n), "weights")
    if state_hist is None:
        state_hist = torch.empty((S, T, d + 2), dtype=torch.float64, device=dev)
    _require_gpu(state_hist)
    _Online._f64(state_hist, (S, T, d + 2), "state_hist")
    rows = _Online._i32(rows, (T, 2), "rows", dev)
    orders = _Online._i32(orders, (T, n), "orders", dev)
    counts = _Online._i32(counts, (S, T, 4), "counts", dev, optional=False)
    info = _Online._i32(info, (S, T, 4), "info", dev, optional=False, zero=True)
    _lib.check(L.rlvi_online_stream_f64(_ptr(X), _ptr(y), _ptr(X_test), _ptr(y_test), _ptr(rows), _ptr(orders), T, n,
                                        m, d, (ctypes.c_int32 * S)(*codes), (ctypes.c_double * S)(*eps), S,
                                        float(alpha), float(tol), int(maxiter), _ptr(state_hist), _ptr(counts),
                                        _ptr(weights), _ptr(info), _stream_ptr()), "rlvi_online_stream_f64")
    return state_hist, counts, weights, info


def stream_copy(dst, src):
    """Measurement aid: flat nontemporal 16-B/lane copy of src into dst (same byte count, 16-byte multiples)."""
    nbytes = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() != nbytes:
        raise ValueError("stream_copy: sizes differ")
    _lib.check(_lib.load().rlvi_stream_copy(_ptr(dst), _ptr(src), nbytes, _stream_ptr()), "rlvi_stream_copy")


class _WeightedCE(torch.autograd.Function):
    """loss = mean_i(pi[idx_i] * CE(logits_i, y_i)) with the residual scatter as a side effect
    (train_rlvi.py:89-94); backward hands out the gradient the fused kernel already wrote."""

    @staticmethod
    def forward(ctx, logits, labels, idx, weights, residuals, inv_scale):
        out, grad = mstep_fwd_bwd(logits.detach(), labels, idx, weights, residuals, inv_scale)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, g_loss, _g_out):
        (grad,) = ctx.saved_tensors
        return grad * g_loss.to(grad.dtype), None, None, None, None, None


def select_smallest(losses, k, out=None):
    """mask[i] = 1.0 for the k smallest losses, else 0.0 -- np.argsort(loss)[:k] of the small-loss
    baselines (train_usdnl.py:18-24, train_coteaching.py:18-30) as a weight vector; equal losses in
    index order.  One launch, no host round trip."""
    L = _lib.load()
    _require_gpu(losses)
    _check_f32_vectors("losses", losses)
    if out is None:
        out = torch.empty_like(losses)
    _lib.check(L.rlvi_select_smallest_f32(_ptr(losses), losses.shape[0], int(k), _ptr(out),
                                          _stream_ptr()), "rlvi_select_smallest_f32")
    return out


def topk_hits(logits, labels, ks, out=None):
    """Rows of the batch whose label is among the k largest logits, for every k of `ks` (at most 8): the counts
    behind accuracy(logit, target, topk) of deep-learning/utils.py:65-79.  Returns a device int32 tensor [len(ks)]
    (no host synchronisation here).  RuntimeError when a k exceeds the number of classes, as torch.topk raises."""
    L = _lib.load()
    _require_gpu(logits, labels)
    if logits.dim() != 2:
        raise ValueError("logits must be [B, C]")
    B, C = logits.shape
    ks = [int(k) for k in ks]
    if not ks or len(ks) > 8:
        raise ValueError("between one and eight values of k per call")
    if max(ks) > C or min(ks) < 1:
        raise RuntimeError("selected index k out of range")
    logits, labels = _as_logits(logits), _as_int64(labels)
    if out is None:
        out = torch.empty(len(ks), dtype=torch.int32, device=logits.device)
    karr = (ctypes.c_int32 * len(ks))(*ks)
    fn = _entry(L, "topk_hits", logits.dtype)
    _lib.check(fn(_ptr(logits), logits.stride(0), _ptr(labels), B, C, karr, len(ks), _ptr(out), _stream_ptr()),
               "rlvi_topk_hits")
    return out


def per_sample_ce(logits, labels, ws=None):
    """F.cross_entropy(logits, labels, reduction='none') by the streaming kernel (forward only)."""
    B = logits.shape[0]
    rows = torch.empty(B, dtype=torch.float32, device=logits.device)
    ones = torch.ones(B, dtype=torch.float32, device=logits.device)
    mstep_fwd_bwd(logits, labels, None, ones, rows, want_grad=False, ws=ws)
    return rows


class _SelectedCE(torch.autograd.Function):
    """loss = inv_scale * sum_i mask_i * CE(logits_i, y_i) for a fixed 0/1 mask; backward hands out
    the gradient the fused kernel wrote (zero rows for unselected samples)."""

    @staticmethod
    def forward(ctx, logits, labels, mask, inv_scale):
        out, grad = mstep_fwd_bwd(logits.detach(), labels, None, mask, None, inv_scale)
        ctx.save_for_backward(grad)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g_loss):
        (grad,) = ctx.saved_tensors
        return grad * g_loss.to(grad.dtype), None, None, None


def selected_cross_entropy(logits, labels, mask, inv_scale):
    return _SelectedCE.apply(logits, labels, mask, inv_scale)


def weighted_cross_entropy(logits, labels, idx, weights, residuals, inv_scale=None):
    """Autograd entry: returns (loss 0-dim tensor, out[4])."""
    return _WeightedCE.apply(logits, labels, idx, weights, residuals, inv_scale)


def _jocor_blocks(logits1, logits2, labels):
    """Both blocks in one native dtype (their own if they share one, else fp32), unit column stride; int64 labels."""
    _require_gpu(logits1, logits2, labels)
    if logits1.dim() != 2 or logits1.shape != logits2.shape:
        raise ValueError("logits1 and logits2 must both be [B, C]")
    if labels.dim() != 1 or labels.shape[0] != logits1.shape[0]:
        raise ValueError("labels must be a [B] vector")
    if logits1.dtype != logits2.dtype:
        logits1, logits2 = logits1.float(), logits2.float()
    return _as_logits(logits1), _as_logits(logits2), _as_int64(labels)


def jocor_forward(logits1, logits2, labels, k, co_lambda=0.1, out=None, ws=None):
    """Forward of loss_jocor (train_jocor.py:29-43) without autograd: pass 1 + selection.  Returns (out, loss_pick,
    sel): out fp32[4] = {L, K_qp, K_pq, top-1 % of logits1}, loss_pick [B] and the 0/1 selection sel [B], all on the
    device (no host synchronisation).  Blocks as _jocor_blocks leaves them; see include/rlvi_hip.h."""
    L = _lib.load()
    B, C = logits1.shape
    dev = logits1.device
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=dev)
    loss_pick = torch.empty(B, dtype=torch.float32, device=dev)
    sel = torch.empty(B, dtype=torch.float32, device=dev)
    ws = ws or workspace(dev)
    fn = _entry(L, "jocor_fwd", logits1.dtype)
    _lib.check(fn(_ptr(logits1), logits1.stride(0), _ptr(logits2), logits2.stride(0), _ptr(labels), B, C, int(k),
                  float(co_lambda), _ptr(loss_pick), _ptr(sel), _ptr(out), ws.ptr, _stream_ptr()), "rlvi_jocor_fwd")
    return out, loss_pick, sel


def jocor_backward(logits1, logits2, labels, sel, k, co_lambda=0.1, grad_out=None, grad_scale=None,
                   want1=True, want2=True):
    """Backward of loss_jocor into both blocks (pass 2): (grad1, grad2) in the logits' dtype, None where not wanted.
    grad_out / grad_scale: one-element fp32 device tensors (upstream gradient, loss scale) read by the kernel."""
    L = _lib.load()
    B, C = logits1.shape
    dev = logits1.device
    _check_grad_scale(grad_out, dev, "grad_out")
    _check_grad_scale(grad_scale, dev)
    g1 = torch.empty((B, C), dtype=logits1.dtype, device=dev) if want1 else None
    g2 = torch.empty((B, C), dtype=logits1.dtype, device=dev) if want2 else None
    fn = _entry(L, "jocor_bwd", logits1.dtype)
    _lib.check(fn(_ptr(logits1), logits1.stride(0), _ptr(logits2), logits2.stride(0), _ptr(labels), _ptr(sel), B, C,
                  int(k), float(co_lambda), _ptr(grad_out), _ptr(grad_scale), _ptr(g1), C if want1 else 0, _ptr(g2),
                  C if want2 else 0, _stream_ptr()), "rlvi_jocor_bwd")
    return g1, g2


class _JoCoRLoss(torch.autograd.Function):
    """L = mean of the k smallest loss_pick (train_jocor.py:29-43); backward = pass 2 with autograd's upstream gradient
    read on the device (a GradScaler's scale arrives the same way: scaler.scale(L) multiplies it in)."""

    @staticmethod
    def forward(ctx, logits1, logits2, labels, k, co_lambda, ws, out):
        out, _, sel = jocor_forward(logits1.detach(), logits2.detach(), labels, k, co_lambda, out=out, ws=ws)
        ctx.save_for_backward(logits1, logits2, labels, sel)
        ctx.k, ctx.co_lambda = k, co_lambda
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        z1, z2, labels, sel = ctx.saved_tensors
        g = g.detach()
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        g1, g2 = jocor_backward(z1.detach(), z2.detach(), labels, sel, ctx.k, ctx.co_lambda, grad_out=g,
                                want1=ctx.needs_input_grad[0], want2=ctx.needs_input_grad[1])
        return g1, g2, None, None, None, None, None


def jocor_num_remember(forget_rate, B):
    """k of train_jocor.py:38-40: int((1 - forget_rate) * B) as ind_sorted[:k] takes it (a negative k drops |k|)."""
    k = int((1 - forget_rate) * B)
    return max(B + k, 0) if k < 0 else min(k, B)


def jocor_loss(logits1, logits2, labels, forget_rate, co_lambda=0.1, ws=None, out=None, check=True):
    """loss_jocor (deep-learning/methods/train_jocor.py:29-43) on the device: a 0-dim fp32 tensor L with gradients
    for both blocks.  The reference's loss is a CPU tensor (its .cpu() at :34, then argsort on the host); this one
    stays on the logits' device -- train_jocor only calls .backward() on it.  The KL terms are the reference's batch
    means (kl_loss_compute's `if reduce:` with reduce='none', :23), so every row gets the KL gradient.
    Both blocks run in their own dtype if they share one of fp32 / bf16 / fp16, else both in fp32; the gradients come
    back in the inputs' dtypes.  Works under torch.autocast and with a GradScaler (scaler.scale(L).backward()).
    out: optional fp32[4] device tensor that receives {L, K_qp, K_pq, top-1 % of logits1}.  check=True reads the
    device status (one 4-byte copy, a sync as the reference's .cpu() is) and raises on a label out of range; a
    training loop passes False and reads the status once at its end."""
    z1, z2, labels = _jocor_blocks(logits1, logits2, labels)
    k = jocor_num_remember(forget_rate, z1.shape[0])
    ws = ws or workspace(z1.device)
    loss = _JoCoRLoss.apply(z1, z2, labels, k, float(co_lambda), ws, out)
    if check:
        ws.raise_on_status("jocor_loss")
    return loss


def _bare_call(logits, labels, k, out, ws, want_grad):
    """The dtype's BARE entry on checked inputs: (out, w, sel, grad).  grad is the gradient of L in the logits' dtype
    when the shape takes the one-workgroup form (which writes it in the same launch) and want_grad is set, else
    None: the streaming form leaves the gradient to the M-step entry (_BareLoss.backward)."""
    L = _lib.load()
    B, C = logits.shape
    dev = logits.device
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=dev)
    w = torch.empty(B, dtype=torch.float32, device=dev)
    sel = torch.empty(B, dtype=torch.float32, device=dev)
    ws = ws or workspace(dev)
    form = L.rlvi_bare_form(B, C)
    _lib.check(min(form, 0), "rlvi_bare_form")
    grad = torch.empty((B, C), dtype=logits.dtype, device=dev) if (want_grad and form == 1) else None
    fn = _entry(L, "bare_fwd", logits.dtype)
    _lib.check(fn(_ptr(logits), logits.stride(0), _ptr(labels), B, C, float(k), _ptr(w), _ptr(sel), _ptr(out),
                  _ptr(grad), C if grad is not None else 0, ws.ptr, _stream_ptr()), "rlvi_bare_fwd")
    return out, w, sel, grad


def _bare_inputs(logits, labels):
    _require_gpu(logits, labels)
    if logits.dim() != 2:
        raise ValueError("logits must be [B, C]")
    if labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise ValueError("labels must be a [B] vector")
    return _as_logits(logits), _as_int64(labels)


def bare_forward(logits, labels, k=1.0, out=None, ws=None):
    """Forward of BARE's WeightedCCE (train_bare.py:28-57) without autograd.  Returns (out, w, sel): out fp32[4] =
    {L, n_kept, fallback, top-1 %}, w [B] = 1 / n_kept on the kept rows and 0 elsewhere (1 / B everywhere in the
    fallback), sel [B] the 0/1 selection -- all on the device, no host synchronisation.  See include/rlvi_hip.h."""
    logits, labels = _bare_inputs(logits, labels)
    out, w, sel, _ = _bare_call(logits, labels, k, out, ws, False)
    return out, w, sel


class _BareLoss(torch.autograd.Function):
    """L = mean CE of the rows BARE keeps.  The one-workgroup form has written the gradient in the forward launch and
    backward hands it out (as _WeightedCE does); otherwise backward is the streaming M-step entry with weights = w,
    idx = None, inv_scale = 1 (as _SelectedCE), the upstream gradient staying on the device: it multiplies the B
    values of w (fp32 / bf16) or goes in as the kernel's grad_scale (fp16: one rounding of the scaled gradient)."""

    @staticmethod
    def forward(ctx, logits, labels, k, ws, out):
        z = logits.detach()
        out, w, sel, grad = _bare_call(z, labels, k, out, ws, ctx.needs_input_grad[0])
        ctx.fused = grad is not None
        ctx.ws = ws
        if ctx.fused:
            ctx.save_for_backward(grad)
        else:
            ctx.save_for_backward(z, labels, w)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        g = g.detach().to(torch.float32)
        if ctx.fused:
            (grad,) = ctx.saved_tensors
            return grad * g.to(grad.dtype), None, None, None, None
        z, labels, w = ctx.saved_tensors
        if z.dtype == torch.float16:
            _, grad = mstep_fwd_bwd(z, labels, None, w, None, inv_scale=1.0, grad_scale=g.reshape(1), ws=ctx.ws)
        else:
            _, grad = mstep_fwd_bwd(z, labels, None, w * g, None, inv_scale=1.0, ws=ctx.ws)
        return grad, None, None, None, None


def bare_loss(logits, labels, k=1.0, ws=None, out=None, check=True):
    """WeightedCCE.forward of deep-learning/methods/train_bare.py:28-57 on the device: a 0-dim fp32 tensor L, the mean
    cross-entropy of the rows whose label probability clears its class's batch mean by k batch deviations (of all
    rows when none does), with the gradient for the logits -- none flows through the statistics.  fp32, bf16 and
    fp16 logits run natively (any other dtype as fp32); the gradient comes back in the logits' dtype.  Works under
    torch.autocast and with a GradScaler.  out: optional fp32[4] device tensor that receives {L, n_kept, fallback,
    top-1 %}.  check=True reads the device status (one 4-byte copy and a sync, as the reference's len(prun_idx) is)
    and raises on a label out of range; a training loop passes False and reads the status once at its end."""
    z, labels = _bare_inputs(logits, labels)
    ws = ws or workspace(z.device)
    loss = _BareLoss.apply(z, labels, float(k), ws, out)
    if check:
        ws.raise_on_status("bare_loss")
    return loss


def cdr_covered(params):
    """The tensors CDR's mask covers (train_cdr.py:25,:41): those with dim() in (2, 4), in the order given."""
    return [p for p in params if p.dim() in (2, 4)]


def cdr_num_nonzero(nonzero_ratio, total):
    """nz of train_cdr.py:32: int(nonzero_ratio * num_params), on whatever float type the caller holds (rate_schedule
    holds np.float64).  IndexError for nz == 0, where the reference's top_values[-1] (:34) raises it."""
    nz = int(nonzero_ratio * total)
    if nz == 0:
        raise IndexError("index -1 is out of bounds for dimension 0 with size 0")
    return nz


class CdrMasker:
    """CDR's gradient masking of train_cdr.py:22-44 over a fixed list of parameters, in five launches per call whatever
    their number: masker(nonzero_ratio, clip) finds thr = the int(nonzero_ratio * total)-th largest |p.grad * p| over
    ALL covered parameters by a radix descent (no concatenated copy, no sort: rlvi_amd/csrc/cdr.hip) and overwrites
    every covered p.grad with ((|p * p.grad| >= thr) * clip) * p.grad -- the reference's bits.

    `params`: the parameters in named_parameters() order; those with dim() in (2, 4) are covered, the others are left
    alone.  The masker owns a pinned host table of {p, p.grad, numel} per covered tensor, its device copy, the
    scratch of the descent and the two outputs.  The table is refilled and uploaded only when a data_ptr() changed
    since the last call (optimizer.zero_grad() sets the gradients to None, so backward allocates them anew; the
    caching allocator usually hands the same addresses back); `uploads` counts how often that happened."""

    def __init__(self, params):
        L = _lib.load()
        self.params = cdr_covered(list(params))
        if not self.params:
            raise ValueError("CdrMasker: no parameter with dim() in (2, 4)")
        _require_gpu(*self.params)
        for p in self.params:
            if p.dtype != torch.float32:
                raise TypeError("CdrMasker: fp32 parameters only (the reference has no other; AMP keeps them fp32)")
            if not p.is_contiguous():
                raise ValueError("CdrMasker: a covered parameter is not contiguous")
        dev = self.params[0].device
        if any(p.device != dev for p in self.params):
            raise ValueError("CdrMasker: parameters on more than one device")
        self.nseg = len(self.params)
        self.total = sum(p.numel() for p in self.params)
        if any(p.numel() < 1 for p in self.params):
            raise ValueError("CdrMasker: an empty parameter")
        nbytes = int(L.rlvi_cdr_table_bytes(self.nseg))
        self._host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self._table = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._scratch = torch.empty(int(L.rlvi_cdr_scratch_bytes(self.nseg)), dtype=torch.uint8, device=dev)
        assert self._table.data_ptr() % 16 == 0 and self._scratch.data_ptr() % 16 == 0
        self.thr = torch.zeros((), dtype=torch.float32, device=dev)
        self.kept = torch.zeros((), dtype=torch.int64, device=dev)
        self._n = (ctypes.c_int64 * self.nseg)(*[p.numel() for p in self.params])
        self._ptrs = None
        self._uploaded = None               # event behind the last upload: the host table is free again after it
        self.chunks = 0
        self.uploads = 0

    def _pointers(self):
        """The addresses of every covered parameter and gradient, as the table holds them.  This runs on every call,
        so it looks at no more than the call could not do without: a gradient that is there and contiguous."""
        grads = []
        for p in self.params:
            g = p.grad
            if g is None:
                raise ValueError("CdrMasker: a covered parameter has no gradient (run backward first)")
            if not g.is_contiguous():
                raise ValueError("CdrMasker: a gradient is not contiguous")
            grads.append(g.data_ptr())
        return tuple([p.data_ptr() for p in self.params] + grads)

    def _refresh(self, ptrs):
        L = _lib.load()
        for p in self.params:                # an address changed: look at the tensors behind them properly
            g = p.grad
            if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
                raise ValueError("CdrMasker: a gradient is not an fp32 tensor of its parameter's shape and device")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("CdrMasker: a covered parameter is no longer a contiguous fp32 tensor")
        if self._uploaded is not None:
            self._uploaded.synchronize()
        v = (ctypes.c_void_p * self.nseg)(*ptrs[:self.nseg])
        g = (ctypes.c_void_p * self.nseg)(*ptrs[self.nseg:])
        total, chunks = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(L.rlvi_cdr_table_fill(ctypes.c_void_p(self._host.data_ptr()), v, g, self._n, self.nseg,
                                         ctypes.byref(total), ctypes.byref(chunks)), "rlvi_cdr_table_fill")
        assert total.value == self.total
        self.chunks = chunks.value
        self._table.copy_(self._host, non_blocking=True)
        self._uploaded = torch.cuda.Event()
        self._uploaded.record()
        self._ptrs = ptrs
        self.uploads += 1

    def __call__(self, nonzero_ratio, clip):
        """Mask the gradients in place; returns (thr, kept) as 0-dim device tensors (fp32, int64) owned by the masker
        and overwritten by its next call.  No host synchronisation.  IndexError for int(nonzero_ratio * total) == 0,
        where the reference's top_values[-1] raises it."""
        nz = cdr_num_nonzero(nonzero_ratio, self.total)
        ptrs = self._pointers()
        if ptrs != self._ptrs:
            self._refresh(ptrs)
        rc = _lib.load().rlvi_cdr_mask_f32(_ptr(self._table), self.nseg, self.total, self.chunks, nz, float(clip),
                                           _ptr(self._scratch), self._scratch.numel(), _ptr(self.thr),
                                           _ptr(self.kept), _stream_ptr())
        _lib.check(rc, "rlvi_cdr_mask_f32")
        return self.thr, self.kept


def cdr_mask_(params, nonzero_ratio, clip):
    """One-shot form of CdrMasker: mask the gradients of `params` in place, return (thr, kept).  A training loop keeps
    a CdrMasker instead (its table survives from step to step)."""
    return CdrMasker(params)(nonzero_ratio, clip)
