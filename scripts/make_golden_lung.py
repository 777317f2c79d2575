"""Generate tests/golden/lung_known.npz: the CT preprocessing of the REFERENCE (README step 1) on piecewise-constant phantoms.

The reference's own functions are ast-extracted from its source text and run here: ``savenpy`` and ``cutmask``
(preprocessing.py), ``th_2t``, ``get_l``, ``maximum_3d`` and ``large_connected_domain26`` (util.py).  Libraries the reference
needs and that are not required here are replaced by shims: skimage's 2-D ``measure.label`` by ``ndimage.label`` with a 3x3
structure and cc3d's 26-connected labelling by ``ndimage.label`` with 3x3x3 (both number components by their first pixel in
raster order; every call asserts it), ``measure.regionprops(...).area`` by a bincount, SimpleITK / ``np.save`` by in-memory
dictionaries.  Every intermediate is recorded: both histograms, ``aaa``, ``T``, ``L``, ``L1``, ``L2``, ``Mask``, the box and
the saved volumes.  Only data is written.

Usage: python scripts/make_golden_lung.py --reference PATH_TO_REFERENCE_CHECKOUT [--time]
  --time: also time the shimmed reference path (savenpy, mode 'prepro') on one 512x512x400 synthetic case on the host.
"""
import argparse
import ast
import os
import sys
import time
import types

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "lung_known.npz")


def functions(path, names):
    tree = ast.parse(open(path).read())
    found = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in found) == sorted(names), (path, names)
    return found


def raster_label(a, structure):
    """ndimage.label, checked to number components in the order of their first voxel in raster order."""
    lab, num = ndimage.label(a, structure=structure)
    if num:
        _, first = np.unique(lab.ravel(), return_index=True)
        first = first[1:] if lab.ravel()[first[0]] == 0 else first
        assert np.all(np.diff(first) > 0), "labels are not in raster order of first appearance"
    return lab, num


class Recorder:
    def __init__(self):
        self.files, self.hists, self.calls = {}, [], {}

    def save(self, path, arr):
        self.files[path] = np.array(arr, copy=True)

    def histogram(self, a, *args, **kw):
        h = np.histogram(a, *args, **kw)
        self.hists.append((h[0].copy(), h[1].copy()))
        return h

    def wrap(self, ns, name):
        fn = ns[name]

        def wrapped(*args, **kw):
            out = fn(*args, **kw)
            self.calls.setdefault(name, []).append(([np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in args], out))
            return out
        ns[name] = wrapped


def namespace(ref, rec, ct, label):
    np_shim = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    np_shim.save = rec.save
    np_shim.histogram = rec.histogram
    np_shim.load = lambda path, allow_pickle=False: rec.files[next(k for k in rec.files if k.endswith("_box.npy"))]
    os_shim = types.SimpleNamespace(path=types.SimpleNamespace(exists=lambda p: True, join=os.path.join), mkdir=lambda p: None)
    measure = types.SimpleNamespace(
        label=lambda a, background=0, return_num=False: raster_label(a, np.ones((3, 3))) if return_num else raster_label(a, np.ones((3, 3)))[0],
        regionprops=lambda lab: [types.SimpleNamespace(area=int(c)) for c in np.bincount(lab.ravel())[1:]])
    cc3d = types.SimpleNamespace(connected_components=lambda a, connectivity=26: raster_label(a, np.ones((3, 3, 3)))[0])
    ns = {"np": np_shim, "os": os_shim, "measure": measure, "cc3d": cc3d, "ndimage": ndimage,
          "binary_fill_holes": ndimage.binary_fill_holes, "print": lambda *a, **k: None,
          "load_itk_image": lambda p: ((label if "mask" in p else ct).copy(), [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]),
          "save_itk": lambda image, origin, spacing, filename: rec.save(filename, image)}
    for fn in functions(os.path.join(ref, "util.py"), ("th_2t", "get_l", "maximum_3d", "large_connected_domain26")) + \
            functions(os.path.join(ref, "preprocessing.py"), ("savenpy", "cutmask")):
        exec(compile(ast.Module(body=[fn], type_ignores=[]), "reference", "exec"), ns)
    for name in ("th_2t", "get_l", "maximum_3d", "large_connected_domain26"):
        rec.wrap(ns, name)
    return ns


def run_savenpy(ref, ct, mode):
    """-> dict of the recorded values, or {'raised': exception class name}."""
    rec = Recorder()
    ns = namespace(ref, rec, ct, None)
    local = {}

    def tracer(frame, event, arg):
        if frame.f_code.co_name != "savenpy":
            return None

        def on_return(fr, ev, a):
            if ev == "return":
                local.update(fr.f_locals)
            return on_return
        return on_return
    sys.settrace(tracer)
    try:
        ns["savenpy"]("CASE01data.nii.gz", "prep", format="nii.gz", mode=mode)
        raised = None
    except IndexError as e:
        raised = type(e).__name__
    finally:
        sys.settrace(None)
    out = {"hist1_y": rec.hists[0][0], "hist1_x": rec.hists[0][1], "raised": np.array(raised or "")}
    out["aaa"] = np.array(local["aaa"] if "aaa" in local else np.nan, dtype=np.float64)
    if raised:
        out["L"] = rec.calls["get_l"][0][1]
        out["T"] = np.array(rec.calls["th_2t"][0][1], dtype=np.float64)
        return out
    out["data_cut"] = rec.files[os.path.join("prep", "CASE01data_cut.nii.gz")]
    if mode == "prediction":
        return out
    out["hist2_y"], out["hist2_x"] = rec.hists[1]
    out["T"] = np.array(rec.calls["th_2t"][0][1], dtype=np.float64)
    out["L"] = rec.calls["get_l"][0][1]
    (_, l1), (in2, l2) = rec.calls["maximum_3d"]
    out["L1"], out["L2"], out["LxL1"] = l1, l2, in2[0]
    out["Mask"] = local["Mask"]
    out["box"] = rec.files[os.path.join("prep", "CASE01_box.npy")]
    out["lung_mask"] = rec.files[os.path.join("prep", "CASE01_lung_mask.nii.gz")]
    assert out["box"].dtype == np.int64 and out["box"].shape == (6, 2)
    return out


def run_cutmask(ref, label, box):
    rec = Recorder()
    rec.save(os.path.join("data", "CASE01_box.npy"), box)
    ns = namespace(ref, rec, None, label)
    try:
        ns["cutmask"]("CASE01mask.nii.gz", "prepmask")
    except IndexError as e:
        return {"raised": np.array(type(e).__name__)}
    return {"raised": np.array(""), "mask_cut": rec.files[os.path.join("prepmask", "CASE01mask_cut.nii.gz")],
            "ldc": rec.calls["large_connected_domain26"][0][1]}


# ---- phantoms (HU before the +1024 shift), all piecewise constant ----------------------------------------------------------
def grid(shape):
    return np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")


def ellipse(shape, cx, cy, rx, ry):
    x, y = grid(shape)
    return ((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2 <= 1.0


def lung_values(shape):
    """Diagonal stripes of -1000 .. -850 HU in steps of 2: no empty histogram bin between air and lung, so T falls between
    the lungs and the soft tissue as on a real CT."""
    x, y = grid(shape)
    return (-1000 + 2 * ((x + y) % 76)).astype(np.int16)


def chest(shape, fov=True, lung_scale=1.0, z_profile=True):
    X, Y, Z = shape
    ct = np.full(shape, -1000, np.int16)
    for z in range(Z):
        s = np.full((X, Y), -1000, np.int16)
        if fov:
            s[~ellipse((X, Y), X / 2, Y / 2, X / 2 + 6, Y / 2 + 4)] = -2048
        s[ellipse((X, Y), X / 2, Y / 2, X * 0.45, Y * 0.44)] = 40
        s[ellipse((X, Y), X / 2 + X * 0.3, Y / 2, 7, 9)] = 300          # a bone-like disc
        f = lung_scale * (0.55 + 0.45 * np.sin(np.pi * (z + 0.5) / Z)) if z_profile else lung_scale
        for side in (-1, 1):
            m = ellipse((X, Y), X / 2 - X * 0.05, Y / 2 + side * Y * 0.2, X * 0.24 * f, Y * 0.14 * f)
            s[m] = lung_values((X, Y))[m]
            s[ellipse((X, Y), X / 2 - X * 0.05, Y / 2 + side * Y * 0.2, 3, 3)] = 30     # a vessel: an island inside the hole
        s[ellipse((X, Y), X / 2 - X * 0.3, Y / 2, 5, 5)] = -1000         # the trachea: a small hole
        ct[:, :, z] = s
    return ct


def case_ties(shape):
    X, Y, Z = shape
    ct = np.full(shape, -1000, np.int16)
    lv = lung_values((X, Y))
    for z in range(Z):
        s = np.full((X, Y), -1000, np.int16)
        third = 3 * z // Z
        if third == 0:            # one body, three equal rectangular holes: the top two by raster order
            s[10:X - 10, 10:Y - 10] = 40
            for k, (x0, y0) in enumerate(((25, 20), (25, 110), (100, 60))):
                s[x0:x0 + 50, y0:y0 + 45] = lv[x0:x0 + 50, y0:y0 + 45]
        elif third == 1:          # two bodies of equal area, each with a hole: the first in raster order is img1
            s[10:80, 10:Y - 10] = 40
            s[95:165, 10:Y - 10] = 40
            s[20:70, 30:100] = lv[20:70, 30:100]
            s[105:155, 40:140] = lv[105:155, 40:140]
        else:                     # two 35x35 holes touching only at a corner: one 8-connected hole of 2450 pixels
            s[10:X - 10, 10:Y - 10] = 40
            s[40:75, 40:75] = lv[40:75, 40:75]
            s[75:110, 75:110] = lv[75:110, 75:110]
            s[40:90, 130:180] = lv[40:90, 130:180]
        ct[:, :, z] = s
    return ct


def case_no_lung(shape):
    X, Y, Z = shape
    ct = np.full(shape, -1000, np.int16)
    ct[4:X - 4, 4:Y - 4, :] = 40
    ct[10:20, 10:30, :] = -900             # holes of 200 pixels: none above 2000
    return ct


def label_case(shape):
    X, Y, Z = shape
    lab = np.zeros(shape, np.uint8)
    x, y = grid((X, Y))
    tube = (x - X / 2 + 20) ** 2 + (y - Y / 2) ** 2 <= 6 ** 2
    lab[tube, 2:Z - 2] = 1
    lab[X // 2 - 21:X // 2 - 18, Y // 2 - 1:Y // 2 + 2, 5:8] = 0     # an internal cavity: filled by binary_fill_holes
    lab[X // 2 + 30:X // 2 + 34, Y // 2 + 30:Y // 2 + 34, 4:9] = 1   # a smaller detached blob
    return lab


def label_tie(shape):
    lab = np.zeros(shape, np.uint8)
    lab[10:14, 10:14, 2:6] = 1
    lab[40:44, 60:64, 3:7] = 1            # same size: the reference takes the highest label (argsort, <= 16 components)
    lab[70:72, 20:22, 2:4] = 1
    return lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (preprocessing.py, util.py)")
    ap.add_argument("--time", action="store_true", help="time the shimmed reference on a 512x512x400 case (host)")
    args = ap.parse_args()
    ref = args.reference
    data = {}
    cases = {"a": (chest((176, 200, 24)), "prepro"),
             "b": (chest((176, 190, 12), fov=False, z_profile=False), "prepro"),
             "c": (case_ties((176, 200, 30)), "prepro"),
             "d": (chest((64, 72, 16), lung_scale=0.8), "prediction"),
             "f": (case_no_lung((40, 48, 10)), "prepro")}
    for key, (ct, mode) in cases.items():
        r = run_savenpy(ref, ct, mode)
        data[f"{key}_ct"] = ct
        data[f"{key}_mode"] = np.array(mode)
        for k, v in r.items():
            v = np.asarray(v)
            data[f"{key}_{k}"] = v.astype(np.uint8) if v.dtype == bool else v
    assert np.isfinite(data["a_aaa"]) and np.isnan(data["b_aaa"]) and data["f_raised"] == "IndexError"
    assert data["a_L"].any() and data["b_L"].any() and data["c_L"].any(), "the phantoms must have a lung field"
    for key, lab, box in (("e", label_case((176, 200, 24)), data["a_box"]), ("e2", label_tie((80, 90, 10)), np.array(
            [[5, 75], [3, 80], [1, 9], [0, 80], [0, 90], [0, 10]], np.int64)), ("e3", np.zeros((20, 22, 8), np.uint8), np.array(
            [[0, 20], [0, 22], [0, 8], [0, 20], [0, 22], [0, 8]], np.int64))):
        r = run_cutmask(ref, lab, box)
        data[f"{key}_label"], data[f"{key}_box"] = lab, box
        for k, v in r.items():
            data[f"{key}_{k}"] = np.asarray(v)
    assert data["e3_raised"] == "IndexError" and data["e_raised"] == ""
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    if args.time:
        ct = chest((512, 512, 400))
        t0 = time.perf_counter()
        run_savenpy(ref, ct, "prepro")
        print(f"host reference savenpy (mode 'prepro', shimmed, 512x512x400): {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    main()
