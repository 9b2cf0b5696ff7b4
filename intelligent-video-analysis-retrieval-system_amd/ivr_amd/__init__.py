"""ivr_amd: the HIP-backed pieces of the retrieval system.  The submodules are imported by name (ivr_amd.index, ivr_amd.tower, ...);
the inverted-file index is also reachable from the package itself, resolved on first use so that importing the package stays free of
side effects."""
_IVF = ("IVFFlatIndex", "IndexIVFFlat", "SearchParametersIVF", "METRIC_INNER_PRODUCT", "METRIC_L2")
__all__ = list(_IVF)


def __getattr__(name):
    if name in _IVF:
        from . import ivf
        return getattr(ivf, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
