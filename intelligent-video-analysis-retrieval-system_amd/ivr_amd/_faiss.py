"""The faiss-shaped surface the index classes share: the metric constants, the score of an unused result slot, numpy results over the
device-resident methods, and the typed `params` argument of search()."""
import numpy as np

METRIC_INNER_PRODUCT = 0      # faiss.METRIC_INNER_PRODUCT
METRIC_L2 = 1                 # faiss.METRIC_L2: what faiss.IndexLSH reports, and named so that asking for it elsewhere can be refused
FLT_MAX = np.finfo(np.float32).max      # an unused slot of an inner-product result is (-FLT_MAX, -1)


def require_inner_product(metric, who):
    """The metric argument of the constructors that support inner product only."""
    if metric != METRIC_INNER_PRODUCT:
        what = "METRIC_L2 is not supported" if metric == METRIC_L2 else f"got {metric}"
        raise ValueError(f"{who}: only METRIC_INNER_PRODUCT ({METRIC_INNER_PRODUCT}) is supported, {what}")


def to_numpy(tensors):
    """Device results -> the tuple of numpy arrays faiss returns."""
    return tuple(t.cpu().numpy() for t in tensors)


def search_numpy(index, x, k, **kw):
    """index.search(x, k) over index.search_device(x, k, **kw): (D, I) numpy arrays."""
    return to_numpy(index.search_device(x, k, **kw))


def typed_params(params, cls, owner):
    """The `params` of owner.search(): None, or a `cls` (SearchParametersIVF / SearchParametersHNSW) that names no selector.
    Returns params."""
    if params is not None:
        if not isinstance(params, cls):
            raise ValueError(f"params must be a {cls.__name__}, got {type(params).__name__}")
        if params.sel is not None:
            raise ValueError(f"search: ID selectors are not supported on {owner}")
    return params
