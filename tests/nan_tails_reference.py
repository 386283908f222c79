"""What the tests of SIGSVGD_FLAG_NAN_TAILS share: the length rule of the flag in numpy, the two ways
of padding a ragged batch to one length, the fold of a last-point-padded gradient, and the rough walks the cases use."""
import numpy as np


def lengths(X):
    """[A] int: the index of each path's first point whose channel 0 is NaN, T where there is none"""
    X = np.asarray(X)
    nan = np.isnan(X[:, :, 0])
    return np.where(nan.any(axis=1), nan.argmax(axis=1), X.shape[1]).astype(np.int64)


def pad_nan(paths, T, dtype=None):
    """a list of [L_i, d] paths -> [A, T, d] with NaN in every channel from each path's end on"""
    d = paths[0].shape[1]
    out = np.full((len(paths), T, d), np.nan, dtype=dtype or paths[0].dtype)
    for i, p in enumerate(paths):
        out[i, :len(p)] = p
    return out


def pad_last(paths, T, dtype=None):
    """a list of [L_i, d] paths -> [A, T, d] with each path's last point repeated (exact for the signature kernel)"""
    d = paths[0].shape[1]
    out = np.empty((len(paths), T, d), dtype=dtype or paths[0].dtype)
    for i, p in enumerate(paths):
        out[i, :len(p)] = p
        out[i, len(p):] = p[-1]
    return out


def fold(g, L):
    """the gradient [A, T, d] of a last-point-padded batch -> that of the paths themselves, in the layout the flag gives: the
    copies of the last point add up in row L - 1, the rows from L on are zero"""
    g = np.asarray(g, np.float64)
    out = np.zeros_like(g)
    for i, l in enumerate(L):
        out[i, :l] = g[i, :l]
        out[i, l - 1] += g[i, l:].sum(axis=0)
    return out


def rough_paths(seed, Ls, d, step=0.5, dtype=np.float32):
    """one random walk per length of Ls, steps of `step` * N(0, 1) per channel, rounded once to `dtype` (fp32: the values an
    fp32-I/O launch reads are then the ones an fp64-I/O launch and the oracle read)"""
    rng = np.random.default_rng(seed)
    return [np.cumsum(step * rng.standard_normal((int(L), d)), axis=0).astype(dtype) for L in Ls]
