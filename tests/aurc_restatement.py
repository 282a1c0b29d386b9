"""Independent fp64 numpy restatement of the AURC contract (DESIGN "AURC on the device"), vectorised, with a STABLE sort.

Sort ascending by confidence (-0.0 == +0.0, ties in sample order); e_i = inclusive error count, E = e_{n-1};
group starts S = { i in [0, n-2] : i == 0 or c_i != c_{i-1} } = s_1 < ... < s_m, s_0 = -1;
R_0 = E/n, R_k = (E - e_{s_k}) / (n-1-s_k); cov_0 = 1, cov_k = (n-1-s_k)/n;
AURC = sum_k (R_{k-1}+R_k)/2 (s_k - s_{k-1})/n + R_m (n-2-s_m)/n; AURC_opt = (1/n) sum_{j=1..E} j/(n-E+j);
recall numerators e_{m_k - 1}, m_k = max(1, int(n k / 100))."""
import numpy as np

KS = (1, 2, 5, 10, 20, 30, 40, 50)


def restate(confids, is_error, ks=KS):
    c = np.asarray(confids, dtype=np.float32) + np.float32(0.0)
    r = np.asarray(is_error).astype(np.int64)
    n = c.size
    order = np.argsort(c, kind="stable")
    c, r = c[order], r[order]
    e = np.cumsum(r)
    E = int(e[-1])
    i = np.arange(max(n - 1, 0))
    start = np.ones(i.size, dtype=bool)
    start[1:] = c[1:n - 1] != c[:n - 2]
    s = i[start]
    m = int(s.size)
    risk = np.concatenate(([E / n], (E - e[s]) / (n - 1 - s)))
    cov = np.concatenate(([1.0], (n - 1 - s) / n))
    steps = np.diff(np.concatenate(([-1], s)))
    aurc = float(np.sum((risk[:-1] + risk[1:]) * 0.5 * (steps / n)))
    s_m = int(s[-1]) if m else -1
    if m and n - 2 - s_m > 0:
        aurc += float(risk[-1] * ((n - 2 - s_m) / n))
    j = np.arange(1, E + 1, dtype=np.float64)
    aurc_opt = float(np.sum(j / (n - E + j)) / n)
    cuts = [max(1, int(n * k / 100)) for k in ks]
    return {
        "AURC": aurc, "AURC_opt": aurc_opt, "EAURC": aurc - aurc_opt, "E": E, "m": m, "s_m": s_m,
        "recall_num": [int(e[min(mk, n) - 1]) for mk in cuts], "cuts": cuts,
        "cov": cov, "risk": risk, "sorted_conf": c, "sorted_err": r.astype(np.uint8),
    }
