"""CPU-side checks of the fp16 path: the C entries and their host-side argument checks, the loss-scaling plug-in's
interface and the driver's --amp switch (no compute calls)."""
import ctypes
import inspect

import pytest


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3


def _aligned(buf):
    return (ctypes.addressof(buf) + 255) & ~255


def test_library_exports_the_fp16_entries(lib):
    from rlvi_amd import _lib
    for name in ("rlvi_mstep_fwd_bwd_f16", "rlvi_topk_hits_f16"):
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
    assert lib.rlvi_abi_version() == 3


def test_mstep_f16_argument_errors_without_a_gpu(lib):
    buf = (ctypes.c_char * 8192)()
    p = _aligned(buf)
    f = lib.rlvi_mstep_fwd_bwd_f16
    #   logits ld labels idx weights residuals N B C inv_scale grad_scale grad ldg out ws stream
    assert f(None, 10, p, p, p, p, 8, 8, 10, 0.1, None, p, 10, p, p, None) == E_NULL
    assert f(p, 10, None, p, p, p, 8, 8, 10, 0.1, None, p, 10, p, p, None) == E_NULL
    assert f(p, 10, p, p, p, p, 8, 8, 10, 0.1, None, p, 10, p, None, None) == E_NULL          # no workspace
    assert f(p, 10, p, p, None, p, 8, 8, 10, 0.1, None, p, 10, p, p, None) == E_NULL          # idx without weights
    assert f(p, 4, p, p, p, p, 8, 8, 10, 0.1, None, p, 10, p, p, None) == E_SHAPE             # ld < C
    assert f(p, 10, p, p, p, p, 8, 8, 10, 0.1, None, p, 4, p, p, None) == E_SHAPE             # ldg < C
    assert f(p, 10, p, p, p, p, 8, 0, 10, 0.1, None, p, 10, p, p, None) == E_SHAPE            # B = 0
    assert f(p + 1, 10, p, p, p, p, 8, 8, 10, 0.1, None, p, 10, p, p, None) == E_ALIGN        # odd logits address
    assert f(p, 10, p, p, p, p, 8, 8, 10, 0.1, None, p + 1, 10, p, p, None) == E_ALIGN        # odd gradient address
    assert f(p, 10, p, p, p, p, 8, 8, 10, 0.1, p + 2, p, 10, p, p, None) == E_ALIGN           # misaligned loss scale


def test_topk_f16_argument_errors_without_a_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p = _aligned(buf)
    ks = (ctypes.c_int32 * 2)(1, 5)
    f = lib.rlvi_topk_hits_f16
    assert f(None, 10, p, 8, 10, ks, 2, p, None) == E_NULL
    assert f(p, 10, p, 8, 10, None, 2, p, None) == E_NULL
    assert f(p, 4, p, 8, 10, ks, 2, p, None) == E_SHAPE                                       # ld < C
    assert f(p, 10, p, 8, 3, ks, 2, p, None) == E_SHAPE                                       # k = 5 > C
    assert f(p + 1, 10, p, 8, 10, ks, 2, p, None) == E_ALIGN                                  # odd logits address


def test_train_rlvi_amp_interface():
    import sys
    from rlvi_amd import methods
    import rlvi_amd.methods.train_rlvi_amp  # noqa: F401
    m = sys.modules["rlvi_amd.methods.train_rlvi_amp"]
    assert m.__all__ == ['train_rlvi_amp']
    assert list(inspect.signature(m.train_rlvi_amp).parameters) == [
        "train_loader", "model", "optimizer", "residuals", "weights", "overfit", "threshold", "scaler"]
    assert methods.train_rlvi_amp is m.train_rlvi_amp
    # the plug-in itself keeps the reference's seven parameters, and both share one epoch body
    t = sys.modules["rlvi_amd.methods.train_rlvi"]
    assert list(inspect.signature(t.train_rlvi).parameters)[-1] == "threshold"
    assert m._train_epoch is t._train_epoch


def test_ops_accept_fp16_as_a_native_dtype():
    import torch
    from rlvi_amd import ops
    assert torch.float16 in ops._NATIVE
    assert ops._check_grad_scale(None, torch.device("cpu")) is None
    with pytest.raises(ValueError):
        ops._check_grad_scale(torch.ones(2), torch.device("cpu"))                 # not one value
    with pytest.raises(ValueError):
        ops._check_grad_scale(torch.ones(1, dtype=torch.float16), torch.device("cpu"))
    s = torch.ones(1)
    assert ops._check_grad_scale(s, torch.device("cpu")) is s


def test_driver_accepts_amp(monkeypatch, tmp_path):
    from rlvi_amd import driver
    assert inspect.signature(driver.run).parameters["amp"].default == "none"
    with pytest.raises(ValueError):
        driver.run(amp="fp8")                                                     # refused before any device work
    seen = {}

    def fake_run(**kw):
        seen.update(kw)
        return []
    monkeypatch.setattr(driver, "run", fake_run)
    for mode in ("none", "bf16", "fp16"):
        driver.main(["--amp", mode, "--result_dir", str(tmp_path), "--n_epoch", "2"])
        assert seen["amp"] == mode
    driver.main(["--result_dir", str(tmp_path)])
    assert seen["amp"] == "none"                                                  # the default is unchanged
    with pytest.raises(SystemExit):
        driver.main(["--amp", "fp8", "--result_dir", str(tmp_path)])
