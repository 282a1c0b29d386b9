"""GPU: the device input pipeline of the STF / THAB / CUDAL / WADS datasets against the goldens the reference classes produced
(tools/gen_golden_datasets.py), and its new kernels against tests/datasets_restatement.py at the shapes where they can go wrong.

The standards are those of tests/test_gpu_input_pipeline.py, restated here: every array ``==`` (tests/test_dataset_flavours_cpu.py asserts
the conditions that entitle the inputs to it); with a yaw, xyz and range within 1 float32 ulp and the same occupancy (the golden's
rotation went through BLAS); normals at 2e-6 where the 3x3 xyz neighbourhood is bit-identical."""
import numpy as np
import pytest
import torch

import datasets_restatement as dr
from conftest import golden
from oracle import kitti as okitti
from oracle import normals as onormals
from semanticlidarunc_amd import ops
from semanticlidarunc_amd.dataset import gpu_pipeline

pytestmark = pytest.mark.gpu
ALL_CASES, inputs, mirror_class, table_of = dr.ALL_CASES, dr.inputs, dr.mirror_class, dr.table_of


def _same_images(got, want, ulps=0):
    """Every element equal; ulps = 1: within one float32 ulp of the golden value, the same pixels occupied."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if ulps == 0:
        bad = got != want
    else:
        bad = (np.abs(got - want) > ulps * np.spacing(np.abs(want))) | ((got == 0) != (want == 0))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _normals_agree(nrm, want, xyz, xyz_want):
    """Pixels whose 3x3 xyz neighbourhood is bit-identical to the golden's meet the normals kernel's 2e-6; a differing xyz pixel can change
    its own and its 8 neighbours' derivatives, so the others are at most 9 times the share of differing xyz pixels."""
    differs = np.any(xyz != xyz_want, axis=0)
    touched = np.zeros_like(differs)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, xs = np.nonzero(differs)
            touched[np.clip(ys + dy, 0, differs.shape[0] - 1), np.clip(xs + dx, 0, differs.shape[1] - 1)] = True
    bad = np.any(np.abs(nrm - want) > 2e-6, axis=0)
    assert nrm.shape == want.shape and nrm.dtype == want.dtype and not (bad & ~touched).any(), np.argwhere(bad & ~touched)[:4].tolist()
    assert bad.mean() <= 9 * differs.mean(), (float(bad.mean()), float(differs.mean()))


def _want_normals(name, g):
    if dr.STORES_NORMALS[name]:
        return g["normals"]
    return onormals.build_normal_xyz(np.ascontiguousarray(g["xyz"].transpose(1, 2, 0))).transpose(2, 0, 1).astype(np.float32)


def _dataset(name, t, paths=(("unused.bin", "unused.label"),)):
    cls, _ = mirror_class(name)
    kw = {k: v for k, v in {**dr.BASE_KW[name], **t["kw"]}.items() if k != "remap_adverse_label"}
    ds = cls(list(paths), rotate=t["rotate"], flip=t["flip"], **kw)
    if "remap_adverse_label" in t["kw"]:                     # as train_semantics.py does: set after construction, read at call time
        ds.remap_adverse_label = t["kw"]["remap_adverse_label"]
    return ds


def _scan(name, key):
    arrs, _ = inputs(name)
    return torch.from_numpy(arrs[f"records_{key}"].copy()), torch.from_numpy(arrs[f"label_{key}"].view(np.int32).copy())


def _check(name, got, g, rotated):
    rng, refl, xyz, nrm, sem = [a.cpu().numpy() for a in got]
    ulps = 1 if rotated else 0
    _same_images(rng, g["range"], ulps)
    _same_images(refl, g["reflectivity"])
    _same_images(xyz, g["xyz"], ulps)
    _same_images(sem, g["semantics"])
    assert np.array_equal(rng != 0, g["range"] != 0)                               # occupancy
    _normals_agree(nrm, _want_normals(name, g), xyz, g["xyz"])


@pytest.mark.parametrize("name,tag", ALL_CASES)
def test_scan_projector_matches_the_reference_class(cuda, name, tag):
    _, meta = inputs(name)
    t = meta["tags"][tag]
    g = golden(f"dataset_{name}_{tag}")
    proj = _dataset(name, t).projector(cuda)
    rec, lab = _scan(name, t["scan"])
    aug = (t["angle"], t["do_flip"])
    if tag == "plain_noresize":             # the height depends on the scan: one sample at a time
        out = proj([rec], [lab], augmentation=[aug])
        assert list(out[0].shape[1:]) == t["shape"] and out[4].dtype == torch.int64 and out[0].is_cuda
        _check(name, [a[0] for a in out], g, False)
        return
    out = proj([rec, rec], [lab, lab], augmentation=[aug, (None, False)])
    assert list(out[0].shape) == [2] + t["shape"] and out[2].shape[1] == 3 and out[4].dtype == torch.int64 and out[0].is_cuda
    _check(name, [a[0] for a in out], g, t["angle"] is not None)
    # the second scan of the batch took its own augmentation (none): it is the plain sample of the same scan and keywords
    plain = golden(f"dataset_{name}_plain") if (t["scan"], t["kw"]) == ("a", {}) else g
    _same_images(out[0][1].cpu().numpy(), plain["range"])
    _same_images(out[4][1].cpu().numpy(), plain["semantics"])


@pytest.mark.parametrize("name", ["stf", "cudal"])
def test_resize_after_the_projection(cuda, name):
    """resize=True of the projected datasets: project, resize to (128, 2048), flip -- exact against the restatement."""
    _, meta = inputs(name)
    arrs, _ = inputs(name)
    t = dict(meta["tags"]["flip"], kw={"resize": True})
    want = dr.restate(name, arrs["records_a"].tobytes(), arrs["label_a"].tobytes(), table_of(name), t["kw"], None, True)
    out = _dataset(name, t).projector(cuda)([_scan(name, "a")[0]], [_scan(name, "a")[1]], augmentation=[(None, True)])
    got = [a[0].cpu().numpy() for a in out]
    assert got[0].shape == (1, 128, 2048)
    for k in (0, 1, 2, 4):
        _same_images(got[k], want[k])
    _normals_agree(got[3], want[3], got[2], want[2])


# ---------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------
def _lut(cuda, id_map):
    return gpu_pipeline.id_map_lut(id_map).to(cuda)


def _bad(cuda):
    return torch.zeros(1, dtype=torch.int32, device=cuda)


@pytest.mark.parametrize("h,w", [(1, 1), (5, 37), (3, 64)])
def test_organised_scan_shapes_and_shifts(cuda, h, w):
    id_map = table_of("thab")
    g = np.random.default_rng(100 * h + w)
    rec = g.uniform(-20, 20, (h * w, 4)).astype(np.float32)
    rec[g.uniform(size=h * w) < 0.3] = 0
    keys = np.array(sorted(id_map), dtype=np.uint32)
    label = (keys[g.integers(0, keys.size, h * w)] | (g.integers(0, 99, h * w).astype(np.uint32) << 16)).astype(np.uint32)
    mapped = np.array([id_map[int(l)] for l in label & 0xFFFF])
    rec_d, lab_d, lut, bad = torch.from_numpy(rec).to(cuda), torch.from_numpy(label.view(np.int32)).to(cuda), _lut(cuda, id_map), _bad(cuda)
    for shift in (0, -1, w, 3 * w + 5):
        for flip in (False, True):
            for angle in (None, -73.0):
                want = dr.organised_image(rec, mapped, h, w, flip, shift, angle)
                img, rng = ops.organised_scan(rec_d, lab_d, lut, bad, h, w, flip, shift, angle)
                again = ops.organised_scan(rec_d, lab_d, lut, bad, h, w, flip, shift, angle)
                assert torch.equal(img, again[0]) and torch.equal(rng, again[1])                      # run-to-run bit identity
                ulps = 0 if angle is None else 1
                _same_images(img.cpu().numpy()[..., 0:3], want[..., 0:3].astype(np.float32), ulps)
                _same_images(img.cpu().numpy()[..., 3:5], want[..., 3:5].astype(np.float32))
                _same_images(rng.cpu().numpy(), np.linalg.norm(want[..., 0:3], axis=-1).astype(np.float32), ulps)
    assert int(bad.item()) == 0
    lab_d[0] = 2                                                                                     # 2 is not a key of the table
    ops.organised_scan(rec_d, lab_d, lut, bad, h, w)
    assert int(bad.item()) == 1


def _row_image(h, w, empty, seed, c=5):
    g = np.random.default_rng(seed)
    img = g.uniform(-5, 5, (h, w, c)).astype(np.float32)
    img[g.uniform(size=(h, w)) < 0.6] = 0
    for r in range(h):
        if r in empty:
            img[r] = 0
        elif not img[r].any():
            img[r, w // 2, 3] = 0.5                          # a row may be kept by one non-zero channel of one pixel
    return img


@pytest.mark.parametrize("h,w,empty,oh,ow,flip", [(1, 9, (), 4, 9, False), (7, 33, (0, 6), 5, 20, True), (7, 33, (0, 3, 6), 16, 70, False),
                                                  (6, 64, (), 6, 64, True), (300, 5, tuple(range(0, 300, 3)), 64, 7, False)])
def test_row_compaction_and_resize(cuda, h, w, empty, oh, ow, flip):
    img = _row_image(h, w, empty, 7 * h + w)
    if h == 7:
        img[1] = 0
        img[1, 2, 4] = 3.0                                   # only the label channel is non-zero: the row stays
        img[2] = 0
        img[2, 0, 0] = -0.0                                  # a negative zero is zero: on its own it keeps nothing
        img[2, 1, 1] = 1e-30                                 # its float32 square underflows to 0, and so does the norm: the row goes
    want = dr.resize_rows(img.copy(), oh, ow, flip)
    kept = dr.nonempty_rows(img)
    d, bad = torch.from_numpy(img).to(cuda), _bad(cuda)
    rows = ops.nonempty_rows(d)
    assert int(rows[0].item()) == kept.size and rows[1:1 + kept.size].cpu().tolist() == kept.tolist()
    out = ops.resize_nearest_rows_hwc(d, rows, oh, ow, bad, flip)
    _same_images(out.cpu().numpy(), want)
    assert torch.equal(rows[:1 + kept.size], ops.nonempty_rows(d)[:1 + kept.size]) and torch.equal(out, ops.resize_nearest_rows_hwc(d, rows, oh, ow, bad, flip))
    assert int(bad.item()) == 0


def test_all_rows_empty_raises_at_the_batch_read(cuda):
    d, bad = torch.zeros((5, 12, 5), device=cuda), _bad(cuda)
    with pytest.raises(ValueError):
        dr.resize_rows(np.zeros((5, 12, 5), np.float32), 4, 4)
    rows = ops.nonempty_rows(d)
    out = ops.resize_nearest_rows_hwc(d, rows, 4, 4, bad)
    assert int(rows[0].item()) == 0 and int(bad.item()) == 1 and not out.any()
    # through the projector: returns at the origin with class 0 and intensity 0 leave every row empty
    proj = mirror_class("wads")[0]([], projection=(8, 16)).projector(cuda)
    launched = []
    orig = ops.build_normals
    x, l = torch.zeros(70, 4), torch.zeros(70, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="rows are all empty"):
        proj([x], [l])
    # resize=False reads the row count on the host: it raises there and launches nothing afterwards in that call
    proj = mirror_class("wads")[0]([], projection=(8, 16), resize=False).projector(cuda)
    ops.build_normals = lambda *a, **k: launched.append(1) or orig(*a, **k)
    try:
        with pytest.raises(RuntimeError, match="every image row"):
            proj([x], [l])
    finally:
        ops.build_normals = orig
    assert not launched


@pytest.mark.parametrize("h,w,scale", [(3, 37, 0.0), (3, 37, 0.9), (5, 100, 41.0), (64, 64, 3.0)])
def test_reflectivity_maximum(cuda, h, w, scale):
    """All zeros divides by 1; a maximum below 1 divides by 1; W no multiple of the 64-lane wave."""
    g = np.random.default_rng(h * w)
    img = g.uniform(-2, 2, (h, w, 5)).astype(np.float32)
    img[..., 3] = g.uniform(0, 1, (h, w)).astype(np.float32) * np.float32(scale)
    img[..., 4] = g.integers(0, 20, (h, w))
    if scale:
        img[h - 1, w - 1, 3] = np.float32(scale)             # the maximum sits in the last pixel
    d = torch.from_numpy(img).to(cuda)
    key = ops.channel_max(d, 3)
    assert ops.channel_max_value(key) == float(img[..., 3].max()) and torch.equal(key, ops.channel_max(d, 3))
    outs = [torch.empty((1, h, w), device=cuda), torch.empty((1, h, w), device=cuda), torch.empty((3, h, w), device=cuda),
            torch.empty((3, h, w), device=cuda), torch.empty((1, h, w), dtype=torch.int64, device=cuda)]
    nrm = ops.build_normals(d)
    ops.range_image_split_ex(d, nrm, *outs, refl_max_key=key)
    want = img[..., 3] / np.maximum(img[..., 3].max(), 1.0)
    assert want.dtype == np.float32
    _same_images(outs[1][0].cpu().numpy(), want)
    _same_images(outs[0][0].cpu().numpy(), np.linalg.norm(img[..., 0:3], axis=-1))
    _same_images(outs[4][0].cpu().numpy(), img[..., 4].astype(np.int64))
    first = [o.clone() for o in outs]
    ops.range_image_split_ex(d, nrm, *outs, refl_max_key=key)
    assert all(torch.equal(a, b) for a, b in zip(first, outs))
    # the plain split is the ex split without its two options
    plain = [torch.empty_like(o) for o in outs]
    ops.range_image_split(d, nrm, *plain)
    ops.range_image_split_ex(d, nrm, *outs)
    assert all(torch.equal(a, b) for a, b in zip(plain, outs))
    given = torch.rand((h, w), device=cuda)
    ops.range_image_split_ex(d, nrm, *outs, range_in=given)
    assert torch.equal(outs[0][0], given)


@pytest.mark.parametrize("n", [1, 63, 65])
def test_point_decode_stride_5(cuda, n):
    arrs, _ = inputs("stf")
    order = np.argsort(np.abs(np.linalg.norm(arrs["records_a"][:, 0:3], axis=-1) - 1.8), kind="stable")[:n]       # the points nearest the threshold
    rec, label = np.ascontiguousarray(arrs["records_a"][order]), np.ascontiguousarray(arrs["label_a"][order])
    label[0] = 20
    rec_d, lab_d, bad = torch.from_numpy(rec).to(cuda), torch.from_numpy(label.view(np.int32)).to(cuda), _bad(cuda)
    for remap in (None, (20, 0)):
        for angle in (None, 33.0):
            want = dr.stf_cloud(rec.tobytes(), label.tobytes(), remap is not None, clip=False)
            if angle is not None:
                want[:, 0:3] = okitti.rotate_z(want[:, 0:3], angle)
            pc, valid = ops.point_decode(rec_d, lab_d, bad, None, 255.0, False, remap, 1.8, angle)
            got = pc.cpu().numpy()
            assert np.array_equal(got[:, 3:5], want[:, 3:5])                                          # float32 division, raw labels, remap
            assert np.allclose(got[:, 0:3], want[:, 0:3], rtol=0, atol=1e-15 * np.abs(want[:, 0:3]).max()) if angle is not None else np.array_equal(got[:, 0:3], want[:, 0:3])
            assert np.array_equal(valid.cpu().numpy().astype(bool), dr.clip_keep(rec[:, 0:3]))        # the clip looks at the unrotated float32 norm
            again = ops.point_decode(rec_d, lab_d, bad, None, 255.0, False, remap, 1.8, angle)
            assert torch.equal(pc, again[0]) and torch.equal(valid, again[1])
    assert int(bad.item()) == 0 and ops.point_decode(rec_d, lab_d, bad)[1] is None
    # the masked, table-driven form on 4-float records is slu_kitti_decode
    id_map = table_of("thab")
    lab4 = torch.full((n,), 0x30000 | 10, dtype=torch.int32, device=cuda)
    rec4 = rec_d[:, :4].contiguous()
    assert torch.equal(ops.point_decode(rec4, lab4, bad, _lut(cuda, id_map), rotate_deg=-12.0)[0], ops.kitti_decode(rec4, lab4, _lut(cuda, id_map), bad, -12.0))


def test_projection_skips_clipped_points_and_is_repeatable(cuda):
    """slu_spherical_projection_valid == the projection of the compacted cloud (data range and fixed range); all points valid == the plain one."""
    arrs, _ = inputs("stf")
    rec, label = arrs["records_a"], arrs["label_a"]
    rec_d, lab_d, bad = torch.from_numpy(rec.copy()).to(cuda), torch.from_numpy(label.view(np.int32).copy()).to(cuda), torch.zeros(4, dtype=torch.int32, device=cuda)
    pc, valid = ops.point_decode(rec_d, lab_d, bad, None, 255.0, False, None, 1.8)
    cloud = dr.stf_cloud(rec.tobytes(), label.tobytes())
    for tr in (None, (-0.45, 0.05)):
        want = dr.oproj.spherical_projection(cloud, 32, 256, theta_range=tr)[0]
        img = ops.spherical_projection_valid(pc, valid, 32, 256, tr, False, bad[2:])
        _same_images(img.cpu().numpy(), want)
        assert torch.equal(img, ops.spherical_projection_valid(pc, valid, 32, 256, tr, False, bad[2:]))
    ones = torch.ones_like(valid)
    assert torch.equal(ops.spherical_projection_valid(pc, ones, 32, 256, None, True), ops.spherical_projection(pc, 32, 256, flip=True)[0])
    assert bad.tolist() == [0, 0, 0, 0]


def test_clip_that_removes_every_point_raises(cuda):
    """The reference: theta.min() of an empty array raises ValueError inside spherical_projection; here RuntimeError at the batch read."""
    with pytest.raises(ValueError):
        dr.stf_sample(np.ones((4, 5), np.float32).tobytes(), np.zeros(4, np.uint32).tobytes(), (8, 16), resize=False)
    proj = mirror_class("stf")[0]([], projection=(8, 16), resize=False).projector(cuda)
    with pytest.raises(RuntimeError, match="no point left after the range clip"):
        proj([torch.ones(4, 5)], [torch.zeros(4, dtype=torch.int32)])
    out = proj([torch.full((4, 5), 2.0)], [torch.zeros(4, dtype=torch.int32)])           # |xyz| = 3.46: kept
    assert int((out[0] > 0).sum()) == 1


def test_unknown_label_raises_key_error(cuda):
    proj = mirror_class("cudal")[0]([], projection=(8, 16), resize=False).projector(cuda)
    x = torch.full((4, 4), 2.0)
    proj([x], [torch.full((4,), 2, dtype=torch.int32)])                                   # 2 is a key of CUDAL's table, not of KITTI's
    with pytest.raises(KeyError):
        proj([x], [torch.full((4,), 3, dtype=torch.int32)])


@pytest.mark.parametrize("name", ["stf", "thab"])
def test_gpu_loader_with_workers_equals_the_per_sample_path(cuda, tmp_path, name):
    arrs, meta = inputs(name)
    rec, label = arrs["records_a"], arrs["label_a"]
    paths = []
    for k in range(3):
        fb, fl = tmp_path / f"{k:06d}.bin", tmp_path / f"{k:06d}.label"
        if name == "thab":
            r = np.roll(rec.reshape(128, 2048, 4), 100 * k, axis=0).reshape(-1, 4)
            l = np.roll(label.reshape(128, 2048), 100 * k, axis=0).reshape(-1)
        else:
            r, l = rec[: rec.shape[0] - 3000 * k], label[: rec.shape[0] - 3000 * k]
        np.ascontiguousarray(r).tofile(fb)
        np.ascontiguousarray(l).tofile(fl)
        paths.append((str(fb), str(fl)))
    ds = _dataset(name, meta["tags"]["plain"], paths)
    singles = [ds[k] for k in range(3)]
    assert all(not t.is_cuda for t in singles[0]) and singles[0][4].dtype == torch.int64
    _same_images(singles[0][0].numpy(), golden(f"dataset_{name}_plain")["range"])
    loader = ds.gpu_loader(device=cuda, batch_size=2, shuffle=False, num_workers=2)
    batches = list(loader)
    assert len(loader) == 2 and [b[0].shape[0] for b in batches] == [2, 1] and all(t.is_cuda for t in batches[0])
    flat = [[t[i].cpu() for t in b] for b in batches for i in range(b[0].shape[0])]
    for one, two in zip(singles, flat):
        assert all(torch.equal(a, b) for a, b in zip(one, two))
