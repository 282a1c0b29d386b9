"""CPU: the fixtures, the restatement and the host side of the STF / THAB / CUDAL / WADS input pipelines.

* tests/datasets_restatement.py reproduces every golden array (the goldens are the reference classes' own outputs,
  tools/gen_golden_datasets.py); xyz / range within 1 float32 ulp where a yaw went through BLAS, everything else ``==``;
* the inputs meet the conditions under which the GPU test compares with ``==`` (tests/projection_cases.py: no point within 2^-40 rad of a
  bin edge, no pixel with two equal ranges), and hold the cases each loader's special rule can get wrong;
* the mirror modules' label tables, constructor signatures and random draws are the reference's;
* what the host refuses."""
import ast
import inspect

import numpy as np
import pytest
import torch

import datasets_restatement as dr
import projection_cases as pcs
from conftest import golden
from semanticlidarunc_amd.dataset import gpu_pipeline
from semanticlidarunc_amd.dataset.definitions import id_map as kitti_id_map

DATASETS, ALL_CASES = dr.DATASETS, dr.ALL_CASES
mirror_class, inputs, id_maps, table_of = dr.mirror_class, dr.inputs, dr.id_maps, dr.table_of


def _ulp_close(got, want):
    return not ((np.abs(got - want) > np.spacing(np.abs(want))) | ((got == 0) != (want == 0))).any()


@pytest.mark.parametrize("name,tag", ALL_CASES)
def test_restatement_reproduces_the_reference_outputs(name, tag):
    arrs, meta = inputs(name)
    t = meta["tags"][tag]
    g = golden(f"dataset_{name}_{tag}")
    mine = dr.restate(name, arrs[f"records_{t['scan']}"].tobytes(), arrs[f"label_{t['scan']}"].tobytes(), table_of(name), t["kw"], t["angle"], t["do_flip"])
    assert list(mine[0].shape) == t["shape"]
    for nme, b in zip(dr.NAMES, mine):
        if nme == "normals" and not dr.STORES_NORMALS[name]:
            continue
        a = g[nme]
        assert a.shape == b.shape and a.dtype == b.dtype, nme
        if t["angle"] is not None and nme in ("range", "xyz"):
            assert _ulp_close(b, a), nme
        else:
            assert np.array_equal(a, b), (nme, int((a != b).sum()))


@pytest.mark.parametrize("name,tag", [c for c in ALL_CASES if c[0] != "thab"])
def test_inputs_are_entitled_to_exact_comparison(name, tag):
    arrs, meta = inputs(name)
    t = meta["tags"][tag]
    kw = {**dr.BASE_KW[name], **t["kw"]}
    cloud, tr = dr.projected_cloud(name, arrs[f"records_{t['scan']}"].tobytes(), arrs[f"label_{t['scan']}"].tobytes(), table_of(name), t["angle"], **kw)
    placed = dr.WADS_FULL_PLACED if (name, t["scan"]) == ("wads", "b") else ()
    rep = pcs.edge_report(cloud, kw["projection"][0], kw["projection"][1], theta_range=tr, exempt=placed)
    assert rep.near.size == 0 and rep.near.size <= 1e-4 * cloud.shape[0], rep.near.tolist()       # nothing had to be dropped: share 0 <= 1e-4
    assert rep.tie_pixels.size == 0, rep.tie_pixels.tolist()
    assert min(rep.row_dist, rep.col_dist) > pcs.EPS


def test_stf_scan_holds_the_cases_of_its_rules():
    arrs, meta = inputs("stf")
    rec, label = arrs["records_a"], arrs["label_a"]
    assert rec.shape[1] == 5 and rec.dtype == np.float32
    norms = np.linalg.norm(rec[:, 0:3], axis=-1)
    t = np.float32(1.8)
    below, above = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(4))
    assert (norms == below).any() and (norms == t).any() and (norms == above).any()
    keep = dr.clip_keep(rec[:, 0:3])
    # numpy compares the float32 norms with 1.8 rounded to float32: a norm of exactly np.float32(1.8) stays, its lower neighbour goes
    assert bool(keep[norms == t].all()) and not keep[norms == below].any() and 250 < int((~keep).sum()) < 400
    assert (label > 0xFFFF).any() and (label == 20).any() and ((label & 0xFFFF) == 20).sum() > (label == 20).sum()
    # both theta extremes of the file belong to clipped points: clipping changes the data range, so it moves rows
    theta = pcs.angles(rec[:, 0:3].astype(np.float64))[1]
    assert not keep[np.argmin(theta)] and not keep[np.argmax(theta)]
    assert not np.array_equal(golden("dataset_stf_plain")["semantics"], golden("dataset_stf_plain_noclip")["semantics"])
    sem, sem_remap = golden("dataset_stf_plain")["semantics"], golden("dataset_stf_plain_remap")["semantics"]
    assert (sem == 20).any() and not (sem_remap == 20).any() and np.array_equal(sem_remap, np.where(sem == 20, 0, sem))
    assert (sem > 0xFFFF).any()


def test_thab_cudal_wads_scans_hold_the_cases_of_their_rules():
    _, meta = inputs("thab")
    w = 2048
    shifts = {tag: dr.roll_shift(meta["tags"][tag]["angle"], w) for tag in ("rot", "rotflip")}
    assert shifts["rot"] < 0 and shifts["rotflip"] > w and meta["tags"]["rotflip"]["do_flip"]       # negative, larger than W, flip with roll
    # a shift that lands on .5 needs angle * W / (2 pi) = k + 1/2: no integer angle but 0 gives one; Python's round is half-to-even there
    assert dr.roll_shift(np.pi, 1) == 0 and dr.roll_shift(3 * np.pi, 1) == 2
    arrs, meta = inputs("cudal")
    assert arrs["records_a"][:, 3].max() > 1 and arrs["records_b"][:, 3].max() < 1
    assert golden("dataset_cudal_plain")["reflectivity"].max() == 1.0 and 0 < golden("dataset_cudal_plain_dim")["reflectivity"].max() < 1
    theta = pcs.angles(arrs["records_a"][:, 0:3].astype(np.float64))[1]
    assert (theta > np.pi / 8).any() and (theta < -np.pi / 8).any()
    arrs, meta = inputs("wads")
    cloud, tr = dr.projected_cloud("wads", arrs["records_a"].tobytes(), arrs["label_a"].tobytes(), table_of("wads"))
    img = dr.oproj.spherical_projection(cloud, 32, 256, theta_range=list(tr))[0]
    kept = dr.nonempty_rows(img)
    assert kept[0] > 0 and kept[-1] < 31 and (np.diff(kept) > 1).any()                          # leading, trailing and interior empty rows
    cloud, tr = dr.projected_cloud("wads", arrs["records_b"].tobytes(), arrs["label_b"].tobytes(), table_of("wads"))
    assert dr.nonempty_rows(dr.oproj.spherical_projection(cloud, 32, 256, theta_range=list(tr))[0]).size == 32
    assert meta["tags"]["plain_noresize"]["shape"] == [1, kept.size, 256]


def test_label_tables_equal_the_reference_modules():
    for name in ("cudal", "wads"):
        assert mirror_class(name)[1].id_map == id_maps()[name]
    assert max(id_maps()["wads"].values()) == 20 and id_maps()["cudal"][2] == 12


@pytest.mark.parametrize("name", DATASETS)
def test_constructor_signature_and_attributes_equal_the_reference(name):
    cls, _ = mirror_class(name)
    _, meta = inputs(name)
    sig = inspect.signature(cls.__init__)
    mine = [(p.name, None if p.default is inspect.Parameter.empty else p.default) for p in sig.parameters.values()]
    want = [(n, None if d is None else ast.literal_eval(d)) for n, d in meta["params"]]
    assert mine == want
    if name != "thab":                      # THAB's default id_map prints in the dict's insertion order
        assert str(sig) == meta["signature"]
    ds = cls([("a.bin", "a.label")])
    for n, d in want[2:]:
        if (name, n) != ("thab", "resize"):                 # the reference accepts it and stores nothing
            assert getattr(ds, n) == d, n
    assert len(ds) == 1 and callable(ds.projector) and isinstance(ds._raw, gpu_pipeline.RawScanDataset)
    assert ds._raw.record == (5 if name == "stf" else 4)


@pytest.mark.parametrize("name", DATASETS)
def test_draws_consume_the_generator_like_the_reference(name):
    cls, _ = mirror_class(name)
    _, meta = inputs(name)
    d = meta["draws"]
    proj = cls([("a.bin", "a.label")], rotate=True, flip=True, **dr.BASE_KW[name]).projector(device="cpu")
    np.random.seed(d["seed"])
    got = [proj.draw_augmentation() for _ in d["angles"]]
    assert [int(a) for a, _ in got] == d["angles"] and [f for _, f in got] == d["flips"]
    for tag, t in meta["tags"].items():     # and every tag's own draw, with only the augmentations that tag switches on
        proj = cls([("a.bin", "a.label")], rotate=t["rotate"], flip=t["flip"], **dr.BASE_KW[name]).projector(device="cpu")
        np.random.seed(t["seed"])
        angle, do_flip = proj.draw_augmentation()
        assert (None if angle is None else int(angle)) == t["angle"] and do_flip == t["do_flip"], tag


def test_kitti_draws_are_unchanged():
    proj = gpu_pipeline.ScanProjector(kitti_id_map, (32, 256), rotate=True, flip=True, device="cpu")
    np.random.seed(5)
    got = [proj.draw_augmentation() for _ in range(4)]
    np.random.seed(5)
    want = []
    for _ in range(4):
        a = float(np.random.randint(-180, 180))
        want.append((a, bool(np.random.rand() < 0.5)))
    assert got == want and all(isinstance(a, float) for a, _ in got)


def test_wads_without_resize_refuses_a_batch():
    cls, _ = mirror_class("wads")
    proj = cls([("a.bin", "a.label")] * 2, projection=(32, 256), resize=None).projector(device="cpu")
    x, l = torch.zeros(8, 4), torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="cannot be stacked into a batch"):
        proj([x, x], [l, l])


def test_spec_and_record_validation():
    with pytest.raises(ValueError):
        gpu_pipeline.DatasetSpec(record=6)
    with pytest.raises(ValueError):
        gpu_pipeline.DatasetSpec(organised=(128, 2048))                      # an organised scan needs the roll rotation and an id_map
    with pytest.raises(ValueError):
        gpu_pipeline.ScanProjector(None)
    spec = mirror_class("stf")[0]([], remap_adverse_label=True)._spec()
    assert spec.remap == (20, 0) and spec.clip == 1.8 and spec.record == 5 and spec.id_map is None and not spec.label_mask
    with pytest.raises(Exception):
        spec.record = 4                                                       # frozen
    assert gpu_pipeline.RawScanDataset([]).record == 4
