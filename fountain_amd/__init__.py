"""fountain_amd: MI355X-native path-tracing core behind akofke/fountain's render()."""
from . import _abi
from .api import (Backend, DirectLightingIntegrator, Film, FountainError, PathIntegrator, PbrtScene, PerspectiveCamera,
                  RandomSampler, SamplerIntegrator, Scene, SceneBuilder, Transform, WhittedIntegrator, default_backend, film_resolve_device, load_ply,
                  load_ply_ascii, make_rays, read_exr, write_exr)
from .filters import Filter, render_filtered
from .subdiv import loop_subdivide, loop_subdivide_cpu

__all__ = ["Backend", "DirectLightingIntegrator", "Film", "Filter", "render_filtered", "DisplayParams", "write_png", "BloomParams", "VectorBlurParams", "MetricsParams", "compare", "compare_cpu", "compare_device", "loop_subdivide", "loop_subdivide_cpu", "FountainError", "PathIntegrator", "PbrtScene", "PerspectiveCamera",
           "RandomSampler", "SamplerIntegrator", "Scene", "SceneBuilder", "Transform", "WhittedIntegrator", "default_backend",
           "film_resolve_device", "load_ply", "load_ply_ascii", "make_rays", "read_exr", "write_exr", "_abi"]


def __getattr__(name):
    # DisplayParams and write_png of fountain_amd.display, imported on first use: the module is also a program
    # (python -m fountain_amd.display), which must not find itself imported already
    if name in ("DisplayParams", "write_png"):
        from . import display
        return getattr(display, name)
    if name == "BloomParams":                    # likewise (python -m fountain_amd.bloom)
        from . import bloom
        return bloom.BloomParams
    if name == "VectorBlurParams":               # likewise (python -m fountain_amd.vectorblur)
        from . import vectorblur
        return vectorblur.VectorBlurParams
    if name in ("MetricsParams", "compare", "compare_cpu", "compare_device"):     # likewise (python -m fountain_amd.metrics)
        from . import metrics
        return getattr(metrics, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
