"""vit-gan_amd: MI355X-native (gfx950) engine for the ViTGAN G/D training hot path.

Python keeps the reference's nn.Module surface (src/v2/modules.py) and drives
hand-written HIP kernels through a C ABI (include/vitgan_hip.h).  Import as
``vit_gan_amd`` (alias module at the repo root).
"""
from . import _lib  # noqa: F401

__all__ = ["_lib", "FeatureMoments", "FrechetDistance", "frechet_distance"]
from .config import Config  # noqa: E402,F401

_METRICS = ("FeatureMoments", "FrechetDistance", "frechet_distance")


def __getattr__(name):  # the Frechet-distance surface (metrics.py), imported on first use: it pulls in torch and the modules
    if name in _METRICS:
        from . import metrics
        return getattr(metrics, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
