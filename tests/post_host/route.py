"""TEST INFRASTRUCTURE ONLY: the numpy statement of the catchment routing (include/lgar.h, lgar_catchment_route /
lgar_catchment_route_grad) -- the queue recurrence itself, row after row -- and the calls of the host
program (post_host.run) that run lgar_py_amd/csrc/lgar_route.hpp -- the fold without a dependence between rows, the hand-over
and the gradient accumulation of the GPU kernels -- over the same data.  Never imported by the product package.
"""
import numpy as np

from post_host import Out, same_bits  # noqa: F401

KMAX = 64  # LGAR_ROUTE_KMAX
SHAPE_B = (1, 63, 64, 65, 257)
SHAPE_K = (1, 2, 5, 8, 64)


def shape_T(K):
    return sorted({0, 1, K - 1, K, K + 1, 11})


def _per_catchment(g, B):
    """ordinates in the device layout, [K] (shared) or [K, B], as [K, B]"""
    g = np.asarray(g, dtype=np.float64)
    return np.repeat(g[:, None], B, axis=1) if g.ndim == 1 else g


def route_ref(x, g, q_in=None):
    """The definition as it is written: for every row t, q[i] += g[i] * x[t] for all i (one rounded product, one rounded add),
    y[t] = q[0], the queue shifts down and +0.0 enters at the top.  x [T, B], g [K] or [K, B], q_in [K, B] or None = zeros.
    Returns (y [T, B], q_out [K, B])."""
    x = np.asarray(x, dtype=np.float64)
    T, B = x.shape
    G = _per_catchment(g, B)
    K = G.shape[0]
    q = np.zeros((K, B)) if q_in is None else np.array(q_in, dtype=np.float64).reshape(K, B)
    y = np.zeros((T, B))
    with np.errstate(all="ignore"):
        for t in range(T):
            q = q + G * x[t][None, :]
            y[t] = q[0]
            q[:-1] = q[1:]
            q[-1] = 0.0
    return y, q


def adjoint_ref(gy, g):
    """gx[t] = the fold of g[k] * gy[t + k] from k = min(K - 1, T - 1 - t) down to 0 from +0.0: the recurrence over the rows in
    reverse order with a zero queue."""
    gy = np.asarray(gy, dtype=np.float64)
    return route_ref(gy[::-1], g)[0][::-1].copy()


def ordinate_grad_ref(x, gy, K):
    """gg[k, b] = sum_{t = k}^{T - 1} gy[t, b] * x[t - k, b], from +0.0 in increasing t, plain fp64 products and adds."""
    x, gy = np.asarray(x, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    T, B = x.shape
    gg = np.zeros((K, B))
    with np.errstate(all="ignore"):
        for t in range(T):
            k = np.arange(min(t, K - 1) + 1)
            gg[k] = gg[k] + gy[t][None, :] * x[t - k]
    return gg


def dense_conv(x, g):
    """The convolution by numpy's own arithmetic in another order (k upward), for bounds: y[t] = sum_k g[k] x[t - k]."""
    T, B = x.shape
    G = _per_catchment(g, B)
    y = np.zeros((T, B))
    for k in range(min(G.shape[0], T)):
        y[k:] += G[k][None, :] * x[:T - k]
    return y


def mixed_data(rng, T, B, K, per):
    """x, gy [T, B], g ([K, B] or [K]) and q_in [K, B] of mixed signs over several decades, with a NaN and a -0.0 in x (in its
    first and last rows where there are any) and a -0.0 ordinate."""
    def draw(*shape):
        return (rng.random(shape) - 0.4) * 10.0 ** rng.integers(-3, 3, shape)
    x, gy, q_in = draw(T, B), draw(T, B), draw(K, B)
    g = draw(K, B) if per else draw(K)
    if T:
        x[0, B // 2] = -0.0
        x[T - 1, 0] = np.nan
        if T > 2:
            x[1, B - 1] = -0.0
    if per:
        g[K - 1, ::3] = -0.0
    q_in[0, B - 1] = -0.0
    return x, gy, g, q_in


def case(c):
    """c: a dict with mode ("forward", "reverse" or "grad"), x [T, B]; forward / reverse: g ([K] shared or [K, B]) and, forward
    only, optionally q_in [K, B]; grad: gy [T, B] and K.  The case of post_host.run that gives (y, q_out), (y, None) or
    (g_out, None)."""
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    x = f64(c["x"])
    T, B = x.shape
    if c["mode"] == "grad":
        gy, g_out = f64(c["gy"]), Out(np.float64, int(c["K"]), B)
        assert gy.shape == (T, B)
        return [("catchment_route_grad", [T, B, int(c["K"])], [x, gy, g_out])], (g_out, None)
    g, forward = f64(c["g"]), c["mode"] == "forward"
    K = g.shape[0]
    assert g.ndim == 1 or g.shape == (K, B)
    q_in = None if c.get("q_in") is None else f64(c["q_in"])
    assert q_in is None or (forward and q_in.shape == (K, B))
    y, q_out = Out(np.float64, T, B), Out(np.float64, K, B) if forward else None
    return [("catchment_route", [T, B, K, int(g.ndim == 2), int(not forward)], [x, g, q_in, q_out, y])], (y, q_out)
