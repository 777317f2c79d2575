"""Generate tests/golden/parse_known.npz: the ATM'22 airway tree parsing of the REFERENCE on synthetic cases.

The reference's own functions are ast-extracted from the source text of ``atm22_skel_parse.py`` (every function except
``large_connected_domain``, which needs skimage and is not part of the parsing) and run here in the order of
``tree_parsing.py:147-159``; the skeleton is given, as everywhere in this project.  Only data is written: per case the inputs
(label, skeleton), ``skeleton_parse`` / ``cd`` / ``num`` of ``skeleton_parsing``, the volume of ``tree_parsing_func``, the voxel
counts, ``ad_matric`` and trachea of the first round, the number of refinement rounds, and the final volume and ``num``.

The generator asserts what tests/test_parse_*.py rely on: over the set a case with at least three refinement rounds, one
with a node that has two parents, one where mode 'reflect' decides a branch point differently from 'constant', one with removed
small components, extents that are not multiples of 64, a last axis above 128; and in every round of every case a unique
largest label, so the trachea never rests on how a sort breaks a tie.

Usage: python scripts/make_golden_parse.py --reference PATH_TO_REFERENCE_CHECKOUT
"""
import argparse
import ast
import os
import sys

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "parse_known.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))


def reference_functions(ref):
    tree = ast.parse(open(os.path.join(ref, "atm22_skel_parse.py")).read())
    ns = {"np": np, "ndimage": ndimage, "os": os, "print": lambda *a, **k: None}
    for fn in tree.body:
        if isinstance(fn, ast.FunctionDef) and fn.name != "large_connected_domain":
            exec(compile(ast.Module(body=[fn], type_ignores=[]), "reference", "exec"), ns)
    return ns


def segment(a, b):
    m = int(np.abs(np.asarray(b) - np.asarray(a)).max()) + 1
    return np.rint(np.linspace(a, b, m)).astype(int)


def fork_tree(rng, shape, depth, radius, crumbs):
    """A recursively forking tube tree: voxelised segments (the skeleton) with cubes of shrinking half-width around them (the
    label); the trunk starts on face 0 of axis 0; one extra segment joins two tips (a cycle); a few crumbs of 1-3 skeleton
    voxels lie apart from it inside the volume."""
    shape = np.asarray(shape)
    skel = np.zeros(shape, np.uint8)
    label = np.zeros(shape, np.uint8)
    tips = []

    def draw(pts, r):
        for p in pts:
            lo, hi = np.maximum(p - r, 0), np.minimum(p + r + 1, shape)
            label[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
        skel[tuple(pts.T)] = 1

    def grow(a, direction, length, level):
        b = np.clip(np.rint(a + direction * length).astype(int), 1, shape - 2)
        pts = segment(a, b)
        draw(pts, max(radius - level // 2, 1))
        if level + 1 == depth:
            tips.append(b)
            return
        for sign in (-1.0, 1.0):
            turn = rng.normal(size=3)
            turn[0] = abs(turn[0]) * 0.3
            d = direction * 0.8 + sign * turn / np.linalg.norm(turn) * 0.9
            grow(b, d / np.linalg.norm(d), length * 0.72, level + 1)

    start = np.array([0, shape[1] // 2, shape[2] // 2])
    draw(segment(start - [0, 9, 0], start), radius)           # a foot lying in face 0: its voxels see themselves in the mirror
    grow(start, np.array([1.0, 0.0, 0.0]), shape[0] * 0.3, 0)
    order = np.argsort([np.linalg.norm(t - tips[0]) for t in tips])
    draw(segment(tips[0], tips[order[1]]), 1)                 # the cycle
    placed = 0
    while placed < crumbs:
        p = np.array([rng.integers(1, s - 3) for s in shape])
        k = int(rng.integers(1, 4))
        pts = np.stack([p + [0, 0, t] for t in range(k)])
        lo, hi = np.maximum(pts.min(0) - 2, 0), np.minimum(pts.max(0) + 3, shape)
        if not skel[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].any():
            skel[tuple(pts.T)] = 1
            label[tuple(pts.T)] = 1
            placed += 1
    return label, skel


def run_reference(ns, label, skeleton):
    rec = {"label": label.astype(np.uint8), "skeleton": skeleton.astype(np.uint8)}
    flags = {}
    skeleton_parse, cd, num = ns["skeleton_parsing"](skeleton.copy())
    rec["skeleton_parse"], rec["cd"], rec["num0"] = skeleton_parse.astype(np.uint8), cd.astype(np.int16), np.array(num)
    # what the tests rely on, measured on the reference's own intermediate quantities
    s = skeleton.astype(np.float32)
    cube = np.ones((3, 3, 3), np.float32)
    flags["reflect"] = bool((((ndimage.convolve(s, cube) * s) > 3) != ((ndimage.convolve(s, cube, mode="constant") * s) > 3)).any())
    first, n_first = ndimage.label(((ndimage.convolve(s, cube) * s) <= 3) & (s > 0), structure=np.ones((3, 3, 3)))
    flags["small"] = bool((np.bincount(first.ravel())[1:] < 5).any())
    vol = ns["tree_parsing_func"](skeleton_parse, label, cd)
    assert vol.max() == num and num < 32767
    rec["parsing0"] = vol.astype(np.int16)
    rounds, multi = 0, False
    while True:
        counts = np.bincount(vol.ravel(), minlength=num + 1)[1:num + 1]
        assert (counts == counts.max()).sum() == 1, "the largest label is not unique: the trachea would rest on a sort tie"
        trachea = ns["loc_trachea"](vol, num)
        ad = ns["adjacent_map"](vol, num)
        if rounds == 0:
            rec["counts0"], rec["ad0"], rec["trachea0"] = counts.astype(np.int64), ad.astype(np.uint8), np.array(trachea)
        parent_map, children_map, _ = ns["parent_children_map"](ad, trachea, num)
        multi = multi or bool((parent_map.sum(axis=1) > 1).any())
        if ns["whether_refinement"](parent_map, children_map, vol, num, trachea) is not True:
            break
        vol, num = ns["tree_refinement"](parent_map, children_map, vol, num, trachea)
        rounds += 1
    flags["multi"], flags["rounds"] = multi, rounds
    rec["rounds"], rec["parsing"], rec["num"] = np.array(rounds), vol.astype(np.int16), np.array(num)
    return rec, flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (atm22_skel_parse.py)")
    args = ap.parse_args()
    ns = reference_functions(args.reference)
    import skeleton_oracle as so
    rng = np.random.default_rng(20261024)
    cases = [fork_tree(rng, (96, 80, 72), 5, 3, 4), fork_tree(rng, (72, 64, 64), 4, 2, 3)]
    tree, tree_skeleton, _ = so.solved("tree")                # last axis 134, with its pinned skeleton
    cases.append((tree.copy(), tree_skeleton.copy()))
    data, allflags = {}, []
    for ci, (label, skel) in enumerate(cases):
        rec, flags = run_reference(ns, label, skel)
        print(f"case{ci}: shape {label.shape} skeleton {int(skel.sum())} num {int(rec['num0'])} -> {int(rec['num'])} {flags}")
        allflags.append(flags)
        for k, v in rec.items():
            data[f"case{ci}_{k}"] = v
    assert max(f["rounds"] for f in allflags) >= 3
    assert any(f["multi"] for f in allflags)
    assert any(f["reflect"] for f in allflags)
    assert any(f["small"] for f in allflags)
    assert any(any(n % 64 for n in c[0].shape) for c in cases) and any(c[0].shape[2] > 128 for c in cases)
    data["ncase"] = np.array(len(cases))
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
