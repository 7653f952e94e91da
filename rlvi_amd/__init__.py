"""rlvi_amd: MI355X-native (gfx950) RLVI E-step / M-step hot path behind the reference's
`--method=rlvi` plug-in interface.  See DESIGN.md and include/rlvi_hip.h."""
import os as _os

__version__ = "0.2.0"

# Several processes on one node (one per GPU) exchange IPC handles of device memory: RCCL for its own
# buffers, rlvi_amd.dist.setup_peers for the inboxes of the sharded E-step.  The driver stack of this
# platform only supports the dmabuf IPC mode, selected by HSA_ENABLE_IPC_MODE_LEGACY=0; without it
# hipIpcGetMemHandle fails with "invalid argument".  The ROCm runtime reads the variable when it starts
# (the first GPU call of the process), so it is defaulted here, at import time, and never overridden.
_os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

# The robust linear regressions of the reference's comparison (standard-learning/main.py:248-357) beside
# standard.linear_regression, and RRM's logistic regression (main.py:361-470), resolved on first use: importing the
# package stays free of torch.
_ESTIMATORS = {
    "rrm_logistic_regression": ("rrm", "logistic_regression"),
    "rrm_logistic_regression_batch": ("rrm", "logistic_regression_batch"),
    "rrm_linear_regression": ("rrm", "linear_regression"),
    "rrm_linear_regression_batch": ("rrm", "linear_regression_batch"),
    "huber_linear_regression": ("huber", "linear_regression"),
    "huber_linear_regression_batch": ("huber", "linear_regression_batch"),
}
__all__ = sorted(_ESTIMATORS)


def __getattr__(name):
    if name in _ESTIMATORS:
        import importlib
        module, attr = _ESTIMATORS[name]
        return getattr(importlib.import_module("." + module, __name__), attr)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
