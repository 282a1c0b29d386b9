#!/usr/bin/env python
"""Fixtures of the STF / THAB / CUDAL / WADS input pipelines.  Same rules as tools/gen_golden_r02.py: runs ONLY in the build container, on
the CPU, imports the reference read-only from /root/reference, asserts that tests/datasets_restatement.py reproduces the reference classes,
and writes small data-only fixtures under tests/golden/:

    dataset_<name>_input.npz    the raw file contents of the seeded synthetic scans, and `meta` (JSON): the reference constructor's
                                signature, the (angle, flip) it drew for every tag, its draw sequence under one seed
    dataset_<name>_<tag>.npz    the reference class's outputs for that tag (normals left out for THAB and WADS: unpinned anyway)
    dataset_id_maps.json        the CUDAL and WADS label tables as the reference modules hold them

cv2 (resize, Scharr), open3d and torchvision.transforms are absent from the image: cv2's two functions are served by the oracle's
restatements (so the normals and the resize stay "parity unpinned", as for SemanticKITTI), the other two are empty stubs.

    python tools/gen_golden_datasets.py [stf thab cudal wads]
"""
import inspect
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, REF)

from oracle import kitti as okitti, normals as onormals          # noqa: E402

for stub in ("seaborn", "cv2", "open3d"):
    sys.modules.setdefault(stub, types.ModuleType(stub))
cv2 = sys.modules["cv2"]
cv2.COLORMAP_TURBO, cv2.CV_32FC1, cv2.INTER_NEAREST = 20, 5, 0
cv2.Scharr = lambda img, ddepth, dx, dy, scale=1.0: onormals.scharr(img, dx, dy, scale)
cv2.resize = lambda img, size, interpolation=None: okitti.resize_nearest(img, size[1], size[0])
tv = types.ModuleType("torchvision")
tv.transforms = types.ModuleType("torchvision.transforms")
tv.transforms.Compose = lambda ts: ts
tv.transforms.ToTensor = lambda: None
sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms

import datasets_restatement as dr                                # noqa: E402
import projection_cases as pcs                                   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
DRAW_SEED, DRAW_COUNT = 7, 6


def save(name, **arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    print(f"  wrote {name}.npz  {os.path.getsize(path) / 1024:.0f} KiB")


class DrawLog:
    """Wraps the two numpy draws the loaders make (the originals still run: the generator's stream is consumed as ever) and keeps the values."""

    def __enter__(self):
        self.angles, self.flips = [], []
        self._randint, self._choice = np.random.randint, np.random.choice

        def randint(*a, **k):
            v = self._randint(*a, **k)
            self.angles.append(int(v))
            return v

        def choice(*a, **k):
            v = self._choice(*a, **k)
            self.flips.append(bool(v))
            return v
        np.random.randint, np.random.choice = randint, choice
        return self

    def __exit__(self, *exc):
        np.random.randint, np.random.choice = self._randint, self._choice


def ref_class(name):
    mod = __import__(f"dataset.dataloader_semantic_{name.upper()}", fromlist=["x"])
    return getattr(mod, dr.CLASS_OF[name]), mod


def ulp_close(a, b):
    return not ((np.abs(a - b) > np.spacing(np.abs(b))) | ((a == 0) != (b == 0))).any()


def scans_of(name, id_map):
    if name == "stf":
        return {"a": dr.synth_stf()}
    if name == "thab":
        return {"a": dr.synth_thab(id_map)}
    if name == "cudal":
        return {"a": dr.synth_cudal(id_map), "b": dr.synth_cudal(id_map, seed=23, max_intensity=0.7)}
    return {"a": dr.synth_wads(id_map), "b": dr.synth_wads(id_map, seed=24, bands=None)}


def pick_seed(cls, paths, kw, rotate, flip, want_sign):
    """A seed under which the reference draws flip = True (when it draws one) and an angle of the wanted sign (when it draws one)."""
    for seed in range(200):
        np.random.seed(seed)
        with DrawLog() as log:
            try:
                cls(paths, rotate=rotate, flip=flip, **kw)[0]
            except Exception:
                raise
        if flip and not log.flips[0]:
            continue
        if rotate and (log.angles[0] == 0 or (log.angles[0] > 0) != (want_sign > 0)):
            continue
        return seed, (log.angles[0] if rotate else None), (log.flips[0] if flip else False)
    raise RuntimeError("no seed found")


def check_preconditions(name, rec, label, id_map, kw, angle, placed=()):
    """The conditions under which the device image is compared with ==: no point within 2^-40 rad of a bin edge, no pixel with two equal ranges."""
    if name == "thab":
        return
    kw = {**dr.BASE_KW[name], **kw}
    cloud, tr = dr.projected_cloud(name, rec.tobytes(), label.tobytes(), id_map, angle, **kw)
    rep = pcs.edge_report(cloud, kw["projection"][0], kw["projection"][1], theta_range=tr, exempt=placed if name == "wads" else ())
    assert rep.near.size <= 1e-4 * cloud.shape[0] and rep.near.size == 0, (name, rep.near.tolist())
    assert rep.tie_pixels.size == 0, (name, rep.tie_pixels.tolist())


def gen(name, id_maps):
    cls, mod = ref_class(name)
    id_map = {"stf": None, "thab": __import__("dataset.definitions", fromlist=["x"]).id_map, "cudal": id_maps.get("cudal"), "wads": id_maps.get("wads")}[name]
    scans = scans_of(name, id_map)
    sig = inspect.signature(cls.__init__)
    meta = {"signature": str(sig), "params": [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in sig.parameters.values()],
            "tags": {}}
    inputs = {}
    with tempfile.TemporaryDirectory() as td:
        paths = {}
        for key, (rec, label) in scans.items():
            fb, fl = os.path.join(td, f"{key}.bin"), os.path.join(td, f"{key}.label")
            rec.tofile(fb)
            label.tofile(fl)
            paths[key] = [(fb, fl)]
            inputs[f"records_{key}"], inputs[f"label_{key}"] = rec, label
        for k, (tag, scan, extra, rotate, flip) in enumerate(dr.CASES[name]):
            kw = {key: v for key, v in {**dr.BASE_KW[name], **extra}.items() if key != "remap_adverse_label"}
            seed, angle, do_flip = pick_seed(cls, paths[scan], kw, rotate, flip, -1 if tag == "rot" else 1)
            np.random.seed(seed)
            ds = cls(paths[scan], rotate=rotate, flip=flip, **kw)
            if "remap_adverse_label" in extra:                  # train_semantics.py sets the attribute after construction
                ds.remap_adverse_label = extra["remap_adverse_label"]
            ref = [t.numpy() for t in ds[0]]
            rec, label = scans[scan]
            placed = dr.WADS_FULL_PLACED if (name, scan) == ("wads", "b") else ()
            check_preconditions(name, rec, label, id_map, extra, angle, placed)
            mine = dr.restate(name, rec.tobytes(), label.tobytes(), id_map, extra, angle, do_flip)
            out = {}
            for nme, a, b in zip(dr.NAMES, ref, mine):
                assert a.shape == b.shape and a.dtype == b.dtype, (name, tag, nme, a.shape, b.shape)
                if angle is not None and nme in ("range", "xyz"):
                    assert ulp_close(b, a), (name, tag, nme)        # the yaw went through BLAS: 1 float32 ulp, the SemanticKITTI bar
                else:
                    assert np.array_equal(a, b), (name, tag, nme, int((a != b).sum()))
                if nme != "normals" or dr.STORES_NORMALS[name]:
                    out[nme] = a
            save(f"dataset_{name}_{tag}", **out)
            meta["tags"][tag] = {"scan": scan, "kw": extra, "rotate": rotate, "flip": flip, "angle": angle, "do_flip": do_flip, "seed": seed,
                                 "shape": list(ref[0].shape)}
            print(f"    {name} {tag}: angle {angle} flip {do_flip} shape {ref[0].shape}  restatement == reference")
        # the draw sequence of the class with both augmentations on, one seed, consecutive samples
        np.random.seed(DRAW_SEED)
        kw = dict(dr.BASE_KW[name])
        ds = cls(paths["a"], rotate=True, flip=True, **kw)
        with DrawLog() as log:
            for _ in range(DRAW_COUNT):
                ds[0]
        meta["draws"] = {"seed": DRAW_SEED, "angles": log.angles, "flips": log.flips}
    if name == "stf":
        t = np.float32(1.8)
        norms = np.linalg.norm(scans["a"][0][:, 0:3], axis=-1)
        for v in (np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(4))):
            assert (norms == v).any(), "the scan must hold the float32 neighbours of the clip threshold"
        assert (scans["a"][1] > 0xFFFF).any() and (scans["a"][1] == 20).any()
    if name == "wads":
        assert meta["tags"]["plain_noresize"]["shape"][1] < 32 and meta["tags"]["plain_full"]["shape"] == [1, 64, 1024]
    save(f"dataset_{name}_input", meta=np.array(json.dumps(meta)), **inputs)


if __name__ == "__main__":
    names = sys.argv[1:] or ["stf", "thab", "cudal", "wads"]
    tables = {n: {int(k): int(v) for k, v in ref_class(n)[1].id_map.items()} for n in ("cudal", "wads")}
    with open(os.path.join(OUT, "dataset_id_maps.json"), "w") as f:
        json.dump({n: {str(k): v for k, v in sorted(t.items())} for n, t in tables.items()}, f, indent=0)
    for n in names:
        print(f"[{n}]")
        gen(n, tables)
    print("dataset restatements pinned against the reference classes")
