"""numpy restatement of the packed weight images of the encoder unit kernels, from the layout include/slu.h documents ("Packed weights"):

the image of W [R][K] (or [R][K][taps]) with K-chunk kc is [ceil(R / 32)][taps][ceil(K / kc) * kc / 2][64] floats; lane l of (32-row block m, tap t,
K-step k2) holds W[32 m + (l & 31)][2 k2 + (l >> 5)][t], 0 outside the matrix.  slu_shuffle_tail_pack: wpw [Co][C], kc = 32.  slu_fire_pack:
wsq [S][Cin] (kc = 32), then w1 [E1][S] (kc = 16), then w3 [E3][S][9] (kc = 16, taps = 9).

afrag_image is the vectorised form the GPU tests compare against; afrag_image_loops is the sentence above as four loops
(test_afrag_restatement_cpu.py holds the one to the other)."""
import numpy as np

TAIL_KC, FIRE_SQUEEZE_KC, FIRE_EXPAND_KC = 32, 32, 16


def _as_rkt(w):
    w = np.asarray(w, dtype=np.float32)
    return w.reshape(w.shape[0], w.shape[1], -1)


def afrag_dims(rows, k, kc, taps=1):
    """(32-row blocks, taps, K-steps, 64)"""
    return (rows + 31) // 32, taps, (k + kc - 1) // kc * (kc // 2), 64


def afrag_floats(rows, k, kc, taps=1):
    return int(np.prod(afrag_dims(rows, k, kc, taps)))


def afrag_image(w, kc):
    w = _as_rkt(w)
    rows, k, taps = w.shape
    mb, _, ks, _ = afrag_dims(rows, k, kc, taps)
    pad = np.zeros((mb * 32, 2 * ks, taps), dtype=np.float32)
    pad[:rows, :k] = w
    # pad[32 m + j, 2 k2 + h, t] -> image[m, t, k2, 32 h + j]
    return np.ascontiguousarray(pad.reshape(mb, 32, ks, 2, taps).transpose(0, 4, 2, 3, 1)).reshape(-1)


def afrag_image_loops(w, kc):
    w = _as_rkt(w)
    rows, k, taps = w.shape
    mb, _, ks, _ = afrag_dims(rows, k, kc, taps)
    out = np.zeros(mb * taps * ks * 64, dtype=np.float32)
    for m in range(mb):
        for t in range(taps):
            for k2 in range(ks):
                for lane in range(64):
                    row, col = 32 * m + (lane & 31), 2 * k2 + (lane >> 5)
                    if row < rows and col < k:
                        out[((m * taps + t) * ks + k2) * 64 + lane] = w[row, col, t]
    return out


def shuffle_tail_image(wpw):
    return afrag_image(wpw, TAIL_KC)


def fire_image(wsq, w1, w3):
    return np.concatenate([afrag_image(wsq, FIRE_SQUEEZE_KC), afrag_image(w1, FIRE_EXPAND_KC), afrag_image(w3, FIRE_EXPAND_KC)])


# the shapes of the issue: ragged in every padded dimension, one and several 32-row blocks, odd K
SHUFFLE_SHAPES = [(1, 1), (33, 13), (96, 58)]                              # (Co, C)
FIRE_SHAPES = [(1, 1, 1, 1), (13, 10, 20, 36), (96, 16, 64, 64)]           # (Cin, S, E1, E3)


def shuffle_weight(co, c, seed=0):
    return np.random.default_rng(seed + 1000 * co + c).standard_normal((co, c)).astype(np.float32)


def fire_weights(cin, s, e1, e3, seed=0):
    g = np.random.default_rng(seed + 1000 * cin + s)
    return tuple(g.standard_normal(shape).astype(np.float32) for shape in ((s, cin), (e1, s), (e3, s, 3, 3)))
