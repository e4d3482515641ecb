"""MI355X-native kernels and modules of the stereo codec.  Submodules are imported by name (masic_amd.ops, masic_amd.nn, ...);
the classes meant to be used from the package itself are resolved on first access, so `import masic_amd` stays free of torch
and of the HIP library."""


def __getattr__(name):
    if name == "StereoCodec":
        from .stereofile import StereoCodec
        return StereoCodec
    if name == "PatchAligner":
        from .align import PatchAligner
        return PatchAligner
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
