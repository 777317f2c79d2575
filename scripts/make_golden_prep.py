"""Generate tests/golden/prep_known.npz: the stage-2/3 preparation of the REFERENCE on synthetic cases.

The reference's own statements are ast-extracted from its source text and run here: ``neighbor_descriptor`` /
``save_lib_weight`` (lib_weight.py), ``save_weight_break`` (weight_br.py) and the candidate statements of
``AirwayHMData.crop`` / ``AirwayHMData3.crop`` (data.py).  Libraries the reference needs and that are not required here are
replaced by shims: cc3d's 26-connected labelling by ``ndimage.label`` with a 3x3x3 structure (the union of components taken by
save_weight_break does not depend on the numbering), skimage's ``binary_dilation`` by ``ndimage.binary_dilation`` with the
cross, ``skeletonize_3d`` by the skeleton of the synthetic case, file IO by in-memory dictionaries.  scipy's
``distance_transform_edt`` with indices is recorded on tie-heavy volumes as well.  Only data (inputs, outputs) is written.

Usage: python scripts/make_golden_prep.py --reference PATH_TO_REFERENCE_CHECKOUT
"""
import argparse
import ast
import os
import types

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "prep_known.npz")


def functions(path, names):
    tree = ast.parse(open(path).read())
    return [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]


def crop_statements(path):
    """The dis / loc_small / loc_skeleton assignments of AirwayHMData.crop and AirwayHMData3.crop."""
    tree = ast.parse(open(path).read())
    out = {}
    for cls in [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("AirwayHMData", "AirwayHMData3")]:
        crop = next(m for m in cls.body if isinstance(m, ast.FunctionDef) and m.name == "crop")
        stmts = [s for s in crop.body if isinstance(s, ast.Assign) and getattr(s.targets[0], "id", "") in ("dis", "loc_small", "loc_skeleton")]
        assert len(stmts) == 3, cls.name
        out[cls.name] = compile(ast.Module(body=stmts, type_ignores=[]), "data.py", "exec")
    return out


class Store:
    """In-memory stand-in for the files the reference reads and writes."""

    def __init__(self):
        self.files = {}

    def save(self, path, arr):
        self.files[path] = np.asarray(arr)


def shim_namespace(store, case):
    np_shim = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    np_shim.save = store.save
    os_shim = types.SimpleNamespace(path=types.SimpleNamespace(exists=lambda p: True, join=os.path.join),
                                    mkdir=lambda p: None, listdir=lambda p: ["CASE1mask.nii.gz"])
    sitk = types.SimpleNamespace(ReadImage=lambda p: case["label"], GetArrayFromImage=lambda x: x)
    nib = types.SimpleNamespace(load=lambda p: types.SimpleNamespace(get_fdata=lambda: case["pred"][None].astype(np.float64)))
    cc3d = types.SimpleNamespace(connected_components=lambda a, connectivity=26: ndimage.label(a, structure=np.ones((3, 3, 3)))[0])
    return {"np": np_shim, "os": os_shim, "sitk": sitk, "nibabel": nib, "cc3d": cc3d, "ndimage": ndimage, "print": lambda *a, **k: None,
            "skeletonize_3d": lambda label: case["skeleton"],
            "binary_dilation": lambda a: ndimage.binary_dilation(a, structure=ndimage.generate_binary_structure(3, 1)),
            "load_json_file": lambda *a, **k: ["CASE1"]}


def tube_case(rng, shape, n_branches, radius, miss):
    """A synthetic airway-like case: voxelised line segments (skeleton), dilated (label), a prediction that misses parts."""
    skel = np.zeros(shape, np.uint8)
    segs = []
    for _ in range(n_branches):
        a = rng.integers(0, shape, 3)
        b = rng.integers(0, shape, 3)
        m = int(np.abs(b - a).max()) + 1
        pts = np.rint(np.linspace(a, b, m)).astype(int)
        skel[tuple(pts.T)] = 1
        segs.append(pts)
    label = ndimage.binary_dilation(skel, ndimage.generate_binary_structure(3, 1), iterations=radius).astype(np.uint8)
    pred = label.copy()
    for pts in segs:                           # cut a piece out of some branches: missed skeleton in the middle or at a tip
        if rng.random() < miss and len(pts) > 4:
            i = int(rng.integers(0, len(pts) - 2))
            j = min(len(pts), i + int(rng.integers(2, 6)))
            lo, hi = np.maximum(pts[i:j].min(0) - 1, 0), pts[i:j].max(0) + 2
            pred[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 0
    pred &= (rng.random(shape) > 0.02).astype(np.uint8)
    return {"label": label, "skeleton": skel, "pred": pred}


def edt_volumes(rng):
    vols = []
    v = np.ones((9, 10, 11), np.uint8); v[::4, ::3, ::5] = 0; vols.append(v)                 # a lattice: many equidistant sites
    v = np.ones((5, 40, 37), np.uint8); v[rng.random(v.shape) < 0.01] = 0; vols.append(v)
    v = np.ones((16, 17, 18), np.uint8); v[0, 0, 0] = 0; v[15, 16, 17] = 0; v[8, 0, 17] = 0; vols.append(v)
    v = (rng.random((1, 30, 31)) < 0.9).astype(np.uint8); vols.append(v)
    v = np.ones((7, 1, 9), np.uint8); v[3, 0, 4] = 0; vols.append(v)
    v = np.ones((12, 12, 12), np.uint8); v[[0, 0, 11, 11], [0, 11, 0, 11], [6, 6, 6, 6]] = 0; v[6, 6, [0, 11]] = 0; vols.append(v)
    v = (rng.random((20, 13, 6)) < 0.97).astype(np.uint8); vols.append(v)
    return vols


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (data.py, lib_weight.py, weight_br.py)")
    args = ap.parse_args()
    ref = args.reference
    rng = np.random.default_rng(20261016)
    data = {}
    vols = edt_volumes(rng)
    for i, vol in enumerate(vols):
        dist, ind = ndimage.distance_transform_edt(vol, return_indices=True)
        data[f"edt{i}_vol"], data[f"edt{i}_dist"], data[f"edt{i}_ind"] = vol, dist, ind.astype(np.int16)
    crops = crop_statements(os.path.join(ref, "data.py"))
    cases = [tube_case(rng, (5, 40, 37), 4, 1, 0.7), tube_case(rng, (24, 33, 29), 7, 1, 0.8), tube_case(rng, (1, 26, 23), 4, 1, 0.8),
             tube_case(rng, (31, 2, 27), 3, 1, 0.9), tube_case(rng, (18, 21, 40), 6, 2, 0.8)]
    zero = tube_case(rng, (9, 14, 11), 2, 1, 0.0)
    zero["pred"] = zero["label"].copy()                       # nothing missed: maxf == 0 (weight_br.py:141-148)
    cases.append(zero)
    for ci, case in enumerate(cases):
        store = Store()
        ns = shim_namespace(store, case)
        for fn in functions(os.path.join(ref, "lib_weight.py"), ("neighbor_descriptor", "save_lib_weight")) + \
                functions(os.path.join(ref, "weight_br.py"), ("save_weight_break",)):
            exec(compile(ast.Module(body=[fn], type_ignores=[]), "reference", "exec"), ns)
        ns["save_lib_weight"]("mask", "lib")
        lib = store.files.pop(os.path.join("lib", "CASE1.npy"))
        assert lib.dtype == np.float16
        ns["save_weight_break"]("root", "pred", "w_br", "br_skel", "split.json")
        w_br = store.files.pop(os.path.join("w_br", "CASE1.npy"))
        br = store.files.pop(os.path.join("br_skel", "CASE1.npy"))
        assert w_br.dtype == np.float16, w_br.dtype
        assert not store.files, list(store.files)
        cs = {}
        for name, code in crops.items():
            loc = {"label": case["label"], "skeleton": case["skeleton"], "pred": case["pred"].astype(np.float64), "ndimage": ndimage,
                   "np": np}
            exec(code, loc)
            cs[name] = loc
        for k in ("loc_small", "loc_skeleton"):
            assert all(np.array_equal(a, b) for a, b in zip(cs["AirwayHMData"][k], cs["AirwayHMData3"][k]))
        p = f"case{ci}_"
        for k in ("label", "skeleton", "pred"):
            data[p + k] = case[k]
        data[p + "lib"] = lib
        data[p + "w_br"] = w_br
        maxf_zero = br.ndim == 3                              # the reference saved a zero volume instead of a where-triple
        data[p + "maxf_zero"] = np.array(maxf_zero)
        data[p + "loc_break"] = (np.zeros((3, 0)) if maxf_zero else br).astype(np.int16)
        for k in ("loc_small", "loc_skeleton"):
            m = np.zeros(case["label"].shape, bool)
            m[cs["AirwayHMData"][k]] = True
            data[p + k] = m
    data["ncase"], data["nedt"] = np.array(len(cases)), np.array(len(vols))
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
