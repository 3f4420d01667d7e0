"""ROCm-native policy-update path of geometry_rl (HIP kernels for gfx950).  The loss modules are exported lazily: importing the package
itself loads nothing."""

_EXPORTS = {"TRPLLoss": "trpl", "ClipPPOLoss2": "ppo", "KLPENPPOLoss": "klpen", "BCLoss": "bc"}


def __getattr__(name):
    if name in _EXPORTS:
        import importlib
        return getattr(importlib.import_module("." + _EXPORTS[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
