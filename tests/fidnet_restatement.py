"""FIDNet with the ResNet34_point backbone (reference src/baselines/FIDNet/FIDNet.py, ResNet.py) restated as a plain-torch function of a
state_dict, on the CPU in fp32 or fp64, in the reference's own order of operations (interpolate, concatenate, conv_1 on 1024 channels) -- the
yardstick of tests/test_fidnet_cpu.py and tests/test_gpu_fidnet.py, and the seeded helpers they share with tools/gen_golden_fidnet.py.

The goldens hold no weights.  A case is rebuilt from its seed: torch.manual_seed(seed), the model's own default initialisation (which must give the
digest the reference's constructor gave), then cenet_restatement.randomise_bn -- BatchNorm statistics and affines drawn from a generator seeded with
seed + 1 and scaled by the `gain` the generator settled on (stored in the fixture).  The output is LOGITS: a gain is accepted where
1 <= max|logit| <= 20 and some logit deviates from its class's mean over the pixels by at least a quarter of max|logit| (`gain_conditions`).

Logits alone do not hold the whole backbone: zeroing layer4.2.bn2.bias in the reference moves them by 4.5e-4 .. 2.6e-3 of their scale.  Each
fixture therefore also stores digests of the backend's 1024-channel map per channel slice (`backend_digest`)."""
import numpy as np
import torch
import torch.nn.functional as F

from cenet_restatement import randomise_bn, sd_digest  # noqa: F401  (shared with the CENet fixtures: one definition)

KEYS_JSON = "fidnet_point_state_dict_keys.json"
LAYERS = (3, 4, 6, 3)
EPS = 1e-5          # nn.BatchNorm2d default
SLOPE = 0.01        # nn.LeakyReLU default
GAINS = (1.0, 0.95, 0.9, 1.05, 0.85, 1.1)
# channel slices of the backend's output: x, x_1, res_2, res_3, res_4 (ResNet.py:588)
SLICES = (("x", 0, 512), ("x_1", 512, 640), ("res_2", 640, 768), ("res_3", 768, 896), ("res_4", 896, 1024))
N_SAMPLE = 64

# name, nclasses, with_normal, (B, Cin, H, W), seed
CASES = (
    ("fidnet_point_b2_16x64", 20, False, (2, 5, 16, 64), 5101),
    ("fidnet_point_b1_8x40", 20, False, (1, 5, 8, 40), 5102),            # x_4 is 1 x 5: one row, the in == 1 branch of the coordinate map
    ("fidnet_point_normal_c3_16x32", 3, True, (1, 8, 16, 32), 5103),
)
CASE_IDS = [c[0] for c in CASES]
PREFIX = "model."


def keys_label(case):
    return f"FIDNet({case[1]}, 'ResNet34_point', with_normal={case[2]})"


def construct(case, fidnet_cls):
    """The case's model from the given class (the reference's or the package's), default-initialised from the case's seed."""
    torch.manual_seed(case[-1])
    return fidnet_cls(case[1], "ResNet34_point", with_normal=case[2])


def package_model(case):
    from semanticlidarunc_amd.fidnet import FIDNet
    return construct(case, FIDNet)


def case_input(case):
    return torch.randn(*case[3], generator=torch.Generator().manual_seed(case[-1] + 2))


def gain_conditions(logits):
    """(scale, deviation): max|logit| and the largest |logit - mean of its class over the pixels of its image|."""
    scale = float(logits.abs().max())
    dev = float((logits - logits.mean((2, 3), keepdim=True)).abs().max())
    return scale, dev


def gain_ok(logits):
    scale, dev = gain_conditions(logits)
    return 1.0 <= scale <= 20.0 and dev >= 0.25 * scale


def backend_digest(t):
    """Per channel slice of a backend map [B, 1024, H, W]: ([sum, abs-sum] in fp64, N_SAMPLE values at a fixed stride of the flattened slice)."""
    sums, samples = [], []
    for _, lo, hi in SLICES:
        s = t[:, lo:hi].double().reshape(-1)
        sums.append([float(s.sum()), float(s.abs().sum())])
        samples.append(s[:: max(1, s.numel() // N_SAMPLE)][:N_SAMPLE].numpy().copy())
    return np.asarray(sums), np.stack(samples)


# ---- functional restatement ----
def _bn(t, sd, p):
    return F.batch_norm(t, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, EPS)


def _cbr(t, sd, conv, bn):
    return F.leaky_relu(_bn(F.conv2d(t, sd[conv + ".weight"], sd[conv + ".bias"]), sd, bn), SLOPE)


def _block(t, sd, p, stride):
    o = F.leaky_relu(_bn(F.conv2d(t, sd[p + ".conv1.weight"], None, stride=stride, padding=1), sd, p + ".bn1"), SLOPE)
    o = _bn(F.conv2d(o, sd[p + ".conv2.weight"], None, padding=1), sd, p + ".bn2")
    if p + ".downsample.0.weight" in sd:
        t = _bn(F.conv2d(t, sd[p + ".downsample.0.weight"], None, stride=stride), sd, p + ".downsample.1")
    return F.leaky_relu(o + t, SLOPE)


def _layer(t, sd, p, blocks, stride):
    for i in range(blocks):
        t = _block(t, sd, f"{p}.{i}", stride if i == 0 else 1)
    return t


def backend(sd, x):
    """ResNet_34_point._forward_impl (ResNet.py:560-590) over the keys below `backend.`."""
    b = "backend."
    x = _cbr(x, sd, b + "conv1", b + "bn_0")
    x = _cbr(x, sd, b + "conv2", b + "bn")
    x = _cbr(x, sd, b + "conv3", b + "bn_1")
    x = _cbr(x, sd, b + "conv4", b + "bn_2")
    x_1 = _layer(x, sd, b + "layer1", LAYERS[0], 1)
    x_2 = _layer(x_1, sd, b + "layer2", LAYERS[1], 2)
    x_3 = _layer(x_2, sd, b + "layer3", LAYERS[2], 2)
    x_4 = _layer(x_3, sd, b + "layer4", LAYERS[3], 2)
    res = [F.interpolate(t, size=x.shape[2:], mode="bilinear", align_corners=True) for t in (x_2, x_3, x_4)]
    return torch.cat([x, x_1] + res, 1)


def head(sd, t):
    """SemanticHead.forward (ResNet.py:160-170) over the keys below `semantic_head.`."""
    h = "semantic_head."
    t = _cbr(t, sd, h + "conv_1", h + "bn1")
    t = _cbr(t, sd, h + "conv_2", h + "bn2")
    return F.conv2d(t, sd[h + "semantic_output.weight"], sd[h + "semantic_output.bias"])


def forward(sd, x, dtype=torch.float32, want_backend=False):
    """What FIDNet.forward returns: the logits [B, nclasses, H, W]; with want_backend, (logits, the backend's [B, 1024, H, W] map)."""
    sd = {k[len(PREFIX):]: v.detach().to(dtype) for k, v in sd.items() if k.startswith(PREFIX) and v.is_floating_point()}
    with torch.no_grad():
        mid = backend(sd, x.to(dtype))
        out = head(sd, mid)
    return (out, mid) if want_backend else out
