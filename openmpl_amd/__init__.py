"""openmpl_amd -- MI355X-native multi-view pose-lifting forward pass (OpenMPL hot path)."""
__version__ = "0.1.0"


def check_device(device: int = -1, synchronize: bool = True):
    """Raise RuntimeError if a forward on `device` lost a hand-off inside its persistent kernel (its poses are NaN).  Forwards
    are asynchronous, so call this after the LAST batch of a loop (synchronize=True waits for the device first): every other
    batch is covered by the next call into the library, the last one only by this."""
    from . import cabi
    cabi.raise_if_device_error(device, synchronize)


def __getattr__(name):
    # PoseEvaluator lives in a module that imports torch and loads the native library: resolved on first use
    if name == "PoseEvaluator":
        from .evaluate import PoseEvaluator
        return PoseEvaluator
    if name in ("triangulate_rays", "triangulate_rays_robust", "triangulate_pixels", "epipolar_errors", "consistency_weights", "refine_points",
                "reprojection_errors", "refine_cameras", "locate_cameras", "relative_pose", "refine_relative_pose", "bundle_adjust", "refine_poses",
                "bone_lengths", "smooth_tracks"):
        from . import geometry
        return getattr(geometry, name)
    if name == "procrustes_align":
        from .procrustes import procrustes_align
        return procrustes_align
    if name in ("pack_distortion", "undistort_points", "distort_points"):
        from . import inputs
        return getattr(inputs, name)
    if name in ("synthesize_views", "project_points"):
        from . import synth
        return getattr(synth, name)
    if name in ("decode_heatmaps", "render_heatmaps"):
        from . import heatmaps
        return getattr(heatmaps, name)
    if name == "rpsm":
        # the module is callable (openmpl_amd.rpsm(...)); importing it binds this attribute for good
        import importlib
        return importlib.import_module(".rpsm", __name__)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
