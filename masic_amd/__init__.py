"""MI355X-native kernels and modules of the stereo codec.  Submodules are imported by name (masic_amd.ops, masic_amd.nn, ...);
the one class meant to be used from the package itself is resolved on first access, so `import masic_amd` stays free of torch
and of the HIP library."""


def __getattr__(name):
    if name == "StereoCodec":
        from .stereofile import StereoCodec
        return StereoCodec
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
