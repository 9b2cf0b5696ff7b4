"""ivr_amd: the HIP-backed pieces of the retrieval system.  The submodules are imported by name (ivr_amd.index, ivr_amd.tower, ...);
the inverted-file index and the binary / LSH indexes are also reachable from the package itself, resolved on first use so that
importing the package stays free of side effects."""
_IVF = ("IVFFlatIndex", "IndexIVFFlat", "SearchParametersIVF", "METRIC_INNER_PRODUCT", "METRIC_L2")
_BINARY = ("BinaryFlatIndex", "IndexBinaryFlat", "IndexLSH", "lsh_rotation")
__all__ = list(_IVF + _BINARY)


def __getattr__(name):
    if name in _IVF:
        from . import ivf
        return getattr(ivf, name)
    if name in _BINARY:
        from . import binary
        return getattr(binary, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
