"""CPU: slu_head_mc_f32 and slu_groupnorm_stats are exported and typed, and refuse bad arguments before any launch (no GPU is touched:
a launch without one could only come back as SLU_ELAUNCH, -3)."""
import ctypes

from semanticlidarunc_amd import _lib

P = 4096          # a non-null, 16-byte aligned pointer value: never dereferenced by a call that is refused


def _head(lib, x=P, T=2, B=1, cin=16, hw=64, mean=P, rstd=P, gamma=P, beta=P, groups=8, relu=1, w=P, bias=P, c=20, eps=1e-12, p_bar=P, h=P, mi=P,
          preds=P):
    return lib.slu_head_mc_f32(x, T, B, cin, hw, mean, rstd, gamma, beta, groups, relu, w, bias, c, eps, p_bar, h, mi, preds, None)


def test_symbols_are_exported_and_typed():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("slu_head_mc_f32", "slu_groupnorm_stats"):
        assert hasattr(raw, name), f"{name} not exported by libslu_hip.so"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int
    assert len(_lib.SIGNATURES["slu_head_mc_f32"][1]) == 20 and len(_lib.SIGNATURES["slu_groupnorm_stats"][1]) == 9
    assert _lib.load().slu_abi_version() == _lib.ABI_VERSION >= 34


def test_head_mc_f32_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    for null in ("x", "w", "p_bar", "h", "mi", "preds"):
        assert _head(lib, **{null: None}) == -1, null
    assert _head(lib, c=0) == -1 and _head(lib, c=33) == -1
    assert _head(lib, cin=0) == -1
    assert _head(lib, T=0) == -1 and _head(lib, B=0) == -1 and _head(lib, hw=0) == -1
    assert _head(lib, cin=16, groups=3) == -1 and _head(lib, groups=0) == -1          # groups must divide Cin
    assert _head(lib, mean=None) == -1 and _head(lib, rstd=None) == -1                # exactly one of mean / rstd
    assert _head(lib, cin=129, groups=1) == -2                                        # beyond the 128 channels it covers
    assert _head(lib, cin=129, mean=None, rstd=None) == -2


def test_groupnorm_stats_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    ok = dict(x=P, n=2, c=16, hw=64, groups=8, eps=1e-5, mean=P, rstd=P)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.slu_groupnorm_stats(a["x"], a["n"], a["c"], a["hw"], a["groups"], a["eps"], a["mean"], a["rstd"], None)
    for null in ("x", "mean", "rstd"):
        assert call(**{null: None}) == -1, null
    assert call(n=0) == -1 and call(c=0) == -1 and call(hw=0) == -1 and call(groups=0) == -1 and call(groups=5) == -1
