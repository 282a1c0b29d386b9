"""fp64 restatement of temperature scaling (DESIGN "Temperature scaling on the device"), written from the formulae of include/slu.h:
the calibration cache rows, the objective and its derivative by log T, the fp64 minimiser and the Adam loop for given permutations.
numpy only.  tools/gen_golden_temp_scaling.py pins it to the reference; the GPU tests hold the kernels to it.

Where the reference materialises an fp32 tensor between two steps (the probabilities before the clamp and the logarithm) the
restatement rounds to fp32 there as well: log p near 0 magnifies every ulp of p, so this rounding belongs to the definition of a
row.  Everything else is fp64."""
import numpy as np

CLAMP = np.float32(1e-12)          # probabilities are clamped here before the logarithm
T_MIN = np.float32(1e-3)           # temperatures are clamped here


def cache_probs(out, kind):
    """fp32 [B,C,H,W] model output -> the fp32 probabilities the rows are the logarithm of."""
    x = np.asarray(out, dtype=np.float32)
    if kind == "probs":
        return x
    x = x.astype(np.float64)
    if kind == "logits":
        e = np.exp(x - x.max(axis=1, keepdims=True))
        se = np.zeros_like(e[:, 0])
        for c in range(e.shape[1]):                      # class order
            se = se + e[:, c]
        return (e / se[:, None]).astype(np.float32)
    if kind == "log_probs":
        return np.exp(x).astype(np.float32)
    raise ValueError(f"Unknown output kind: {kind}")


def rows_from_probs(probs, labels, ignore_index):
    """fp32 probabilities [B,C,H,W] -> (rows fp32 [N,C], labels int64 [N]): log(max(p, 1e-12)) of the pixels with label != ignore_index
    (all when None) in (b, h, w) order; the logarithm in fp64, rounded to fp32."""
    p = np.maximum(np.asarray(probs, dtype=np.float32), CLAMP)
    v = np.log(p.astype(np.float64)).astype(np.float32)
    c = v.shape[1]
    rows = v.transpose(0, 2, 3, 1).reshape(-1, c)
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    keep = np.ones(lab.shape, dtype=bool) if ignore_index is None else lab != ignore_index
    return rows[keep], lab[keep]


def cache_rows(out, kind, labels, ignore_index):
    """The cache rows of a model output of `kind`: rows_from_probs of cache_probs."""
    return rows_from_probs(cache_probs(out, kind), labels, ignore_index)


def prob_excess(out, kind, probs32):
    """Largest |probs32 - cache_probs(out, kind)| of an fp32 evaluation of the same formula, as a fraction of what fp32 arithmetic allows:
    relative 2^-24 times (|x_c - max x| for the rounded argument of the exponential, 2 for the exponential, C - 1 for the sum, 1 for
    the quotient, 1 for the rounding of the restatement) for logits, 3 * 2^-24 for log-probs, nothing for probabilities."""
    x = np.asarray(out, dtype=np.float64)
    want = cache_probs(out, kind).astype(np.float64)
    err = np.abs(np.asarray(probs32, dtype=np.float64) - want)
    if kind == "probs":
        return 0.0 if not err.any() else np.inf
    units = (np.abs(x - x.max(axis=1, keepdims=True)) + x.shape[1] + 3.0) if kind == "logits" else 3.0
    allowed = 2.0 ** -24 * units * want + 2.0 ** -149      # the second term: a subnormal's spacing
    return float((err / allowed).max())


def temperature(log_t, fp32=True):
    """(T, clamped) for a log-temperature: T = max(exp(log_t), fp32(1e-3)).  fp32: the exponential rounded to fp32, the T of an
    fp32 log-temperature as the kernels and the reference hold it; otherwise unrounded, for the fits that move log T in fp64."""
    et = float(np.exp(np.float64(log_t)))
    if fp32:
        et = float(np.float32(et))
    return max(et, float(T_MIN)), et < float(T_MIN)


def nll_terms(rows, labels, log_t, idx=None, fp32_t=True):
    """per-row (loss, g = d loss / d log T) in fp64 for rows fp32 [N,C] (gathered by idx when given)."""
    x = np.asarray(rows, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    if idx is not None:
        x, y = x[idx], y[idx]
    t, clamped = temperature(log_t, fp32_t)
    s = x / t
    m = s.max(axis=1)
    e = np.exp(s - m[:, None])
    se = e.sum(axis=1)
    r = np.arange(x.shape[0])
    loss = np.log(se) - (s[r, y] - m)
    g = (e * (x[r, y][:, None] - x)).sum(axis=1) / se / t          # (x_y - sum_c p_c x_c) / T
    return loss, np.zeros_like(g) if clamped else g


def nll(rows, labels, log_t, idx=None, fp32_t=True):
    """(loss_sum, g_sum) as Python floats."""
    loss, g = nll_terms(rows, labels, log_t, idx, fp32_t)
    return float(loss.sum()), float(g.sum())


def minimiser(rows, labels, lo=np.log(1e-2), hi=np.log(1e3), iters=200):
    """T64: the temperature at which g_sum changes sign, by bisection on log T (the objective is convex in 1 / T and has one
    stationary point when the rows are neither all right nor all wrong)."""
    glo, ghi = nll(rows, labels, lo, None, False)[1], nll(rows, labels, hi, None, False)[1]
    assert glo < 0.0 < ghi, (glo, ghi)
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        if nll(rows, labels, mid, None, False)[1] < 0.0:
            lo = mid
        else:
            hi = mid
    return float(np.exp(0.5 * (lo + hi)))


def adam_fit(rows, labels, perms, chunk_size, lr=0.05, start_t=1.0, betas=(0.9, 0.999), eps=1e-8):
    """The Adam loop of the fit in fp64: one epoch per permutation in `perms`, one step per chunk of `chunk_size` indices on the
    chunk's mean loss.  -> T."""
    log_t = float(np.log(start_t))
    m = v = 0.0
    step = 0
    n = len(labels)
    for perm in perms:
        perm = np.asarray(perm, dtype=np.int64)
        assert perm.shape == (n,)
        for i in range(0, n, chunk_size):
            idx = perm[i:i + chunk_size]
            grad = nll(rows, labels, log_t, idx, False)[1] / len(idx)
            step += 1
            m = betas[0] * m + (1.0 - betas[0]) * grad
            v = betas[1] * v + (1.0 - betas[1]) * grad * grad
            mhat = m / (1.0 - betas[0] ** step)
            vhat = v / (1.0 - betas[1] ** step)
            log_t -= lr * mhat / (np.sqrt(vhat) + eps)
    return float(np.exp(log_t))


# ---- the cases of the objective's tests: shared by tools/gen_golden_temp_scaling.py (the reference's own fp32 error per case) and the
# GPU test (the kernel's error per case), so that both evaluate the same data --------------------------------------------------------
NLL_NS = (1, 63, 64, 65, 257, 4099)
NLL_CS = (1, 3, 20, 21, 32)
NLL_LOG_TS = tuple(np.float32(np.log(t)) for t in (1e-4, 1.0, 6.3, 50.0))      # the first one is below the clamp
NLL_VARIANTS = ("all", "reversed", "repeated")


def nll_index(variant, n):
    """Gather index of a variant: None (rows 0..n), n-1..0, or n + 7 draws with repetitions."""
    if variant == "all":
        return None
    if variant == "reversed":
        return np.arange(n - 1, -1, -1, dtype=np.int64)
    assert variant == "repeated"
    return np.random.RandomState(4000 + n).randint(0, n, size=n + 7).astype(np.int64)


def nll_case(master_rows, master_labels, n, c):
    """rows [n, c] / labels [n] of a case, cut from the fixture's [4099, 32] rows; labels folded into [0, c)."""
    return np.ascontiguousarray(master_rows[:n, :c]), np.ascontiguousarray(master_labels[:n] % c)


def ulp_distance(a, b):
    """Largest distance in units of the last place between two fp32 arrays (finite values)."""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, np.int64(-(2 ** 31)) - a, a)      # order the bit patterns like the values
    b = np.where(b < 0, np.int64(-(2 ** 31)) - b, b)
    return int(np.abs(a - b).max()) if a.size else 0
