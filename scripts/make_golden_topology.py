"""Generate tests/golden/topology_known.npz: the reference's own airway parser (``ske_and_parse.airway_parse``) on synthetic trees.

The reference's functions are ast-extracted at run time from the source text of ``ours_skel_parse.py`` (``subsection``,
``compute_base_vector``, ``cosine``, ``find_mainpart_index``, ``smooth_points``, ``process_mainairway_points``, ``merging``,
``tree_parsing_func``, ``NDSparseMatrix`` and the method ``Topology_Tree.grade``) and of ``ske_and_parse.py`` (the order rule: the
statements of ``airway_parse`` up to and including its first ``if``).  The few lines of glue in ``sub()``, ``merge()`` and
``airway_parse`` itself are restated here.  Only data is written.

Sort order.  The reference sorts with numpy's default ``argsort``, which is not stable, in ``sub()`` and in ``smooth_points``; the
order among equal axis-2 coordinates then depends on numpy's build and the CPU.  The project's choice is the STABLE sort
(DESIGN.md 3g): the glue here sorts stably and the extracted functions see ``np`` as a forwarding shim whose ``argsort`` is stable.

Stand-ins for third-party calls that are not installed (not checked against skimage):
  skimage.morphology.binary_dilation   scipy.ndimage.binary_dilation, default structure (the 6-neighbour cross), outside = 0
  skimage.morphology.binary_closing    scipy.ndimage.binary_erosion(binary_dilation(x), border_value=True), the same cross
  scipy.ndimage.binary_fill_holes      itself
  util.maximum_3d (cc3d)               oracle/components_oracle.maximum_3d (scipy.ndimage.label)
  skimage.measure.label (2-D)          scipy.ndimage.label with the full 3x3 structure
  skimage.morphology.skeletonize_3d    tests/skeleton_oracle.skeletonize

Per case: label (int16), order, LABEL_TRANS, skeleton, B before and after smoothing, the base vector, the main-part index, the branch
tables of the first and second ``subsection`` and after merging (flattened arrays), the grade strings, cd and the final volume.
One more record, ``nan_*``, holds ``compute_base_vector`` on a volume with an empty slice: a 26-connected LABEL_TRANS has no
empty slice between its extremes, so that path is recorded at the function, not through the whole parser.

Usage: python scripts/make_golden_topology.py --reference PATH_TO_REFERENCE_CHECKOUT
"""
import argparse
import ast
import copy
import os
import sys
import types
import warnings

import numpy as np
from scipy import ndimage
from scipy.interpolate import interp1d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "topology_known.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

OURS = ("subsection", "compute_base_vector", "cosine", "find_mainpart_index", "smooth_points", "process_mainairway_points", "merging",
        "tree_parsing_func", "NDSparseMatrix")


class StableNumpy:
    """``np`` for the extracted functions: numpy, except that ``argsort`` is stable."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, *args, **kw):
        kw["kind"] = "stable"
        return np.argsort(a, *args, **kw)


def reference_functions(ref):
    ns = {"np": StableNumpy(), "copy": copy, "interp1d": interp1d, "ndimage": ndimage, "print": lambda *a, **k: None}
    tree = ast.parse(open(os.path.join(ref, "ours_skel_parse.py")).read())
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in OURS:
            exec(compile(ast.Module(body=[node], type_ignores=[]), "reference", "exec"), ns)
        if isinstance(node, ast.ClassDef) and node.name == "Topology_Tree":
            grade = next(f for f in node.body if isinstance(f, ast.FunctionDef) and f.name == "grade")
            exec(compile(ast.Module(body=[grade], type_ignores=[]), "reference", "exec"), ns)
    assert all(n in ns for n in OURS + ("grade",))
    # the order rule: airway_parse up to its first `if`
    tree = ast.parse(open(os.path.join(ref, "ske_and_parse.py")).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "airway_parse")
    stop = next(i for i, s in enumerate(fn.body) if isinstance(s, ast.If))
    rule = compile(ast.Module(body=fn.body[:stop + 1], type_ignores=[]), "reference", "exec")

    def label2d(a, background=0, return_num=True):
        return ndimage.label(a, structure=np.ones((3, 3)))

    def order_rule(pred):
        env = {"np": np, "measure": types.SimpleNamespace(label=label2d), "pred": pred}
        exec(rule, env)
        return int(env["order"])
    ns["order_rule"] = order_rule
    return ns


def label_trans(label):
    import components_oracle as co
    x = ndimage.binary_fill_holes(ndimage.binary_dilation(label))
    x = ndimage.binary_erosion(ndimage.binary_dilation(x), border_value=True)
    return co.maximum_3d(x)


def flatten(table):
    n = len(table)
    end = np.zeros((n, 3), np.int64)
    for i, b in enumerate(table):
        if "end" in b:
            end[i] = b["end"]
    members = [p for b in table for p in b["member"]]
    return {"index": np.array([b["index"] for b in table], np.int64),
            "fatherindex": np.array([b["fatherindex"] for b in table], np.int64),
            "start": np.array([b["start"] for b in table], np.int64).reshape(n, 3),
            "has_end": np.array(["end" in b for b in table], np.uint8),
            "end": end,
            "member_count": np.array([len(b["member"]) for b in table], np.int64),
            "members": np.array(members, np.int64).reshape(len(members), 3)}


def run_reference(ns, label, merge_t=5):
    import skeleton_oracle as so
    rec, flags = {"label": label.astype(np.int16)}, {}
    order = ns["order_rule"](label)
    n2 = label.shape[2]
    # Topology_Tree.sub()
    LT = label_trans(label)
    skel, _ = so.skeletonize(LT)
    B = np.array(np.where(skel != 0))
    flags["ties"] = bool((B[2].argsort() != B[2].argsort(kind="stable")).any())
    B = B[:, B[2].argsort(kind="stable")]
    B = B.T
    if order == 1:
        B[:, 2] = n2 - B[:, 2]
    B0 = B.copy()
    Bi = ns["subsection"](B, debug=1)
    table0 = copy.deepcopy(Bi)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        basev = ns["compute_base_vector"](LT, order)
        mmm = ns["find_mainpart_index"](B[0, 2], Bi, basev)
    if mmm > 1:
        B = ns["process_mainairway_points"](B, Bi, mmm)
        Bi = ns["subsection"](B, debug=1)
    table1 = copy.deepcopy(Bi)
    flags["multiway"] = max(int((np.array([tuple(b["start"]) for b in Bi]) == np.array(s)).all(axis=1).sum())
                            for s in {tuple(b["start"]) for b in Bi})
    # Topology_Tree.merge()
    Bi = ns["merging"](Bi, merge_t)
    # which kinds of removal happened (on the table before merging): a short leaf; more branches gone than short ones
    lengths = [1 + len(b["member"]) + ("end" in b) for b in table1]
    fathers = [b["fatherindex"] for b in table1]
    flags["leaf_cut"] = any(l <= merge_t and (i + 1) not in fathers[i + 1:] for i, l in enumerate(lengths))
    flags["single_cut"] = len(table1) - len(Bi) > sum(l <= merge_t for l in lengths)
    if order == 1:
        for b in Bi:
            b["start"][2] = n2 - b["start"][2]
            if "end" in b:
                b["end"][2] = n2 - b["end"][2]
            if b["member"] != []:
                member = np.array(b["member"])
                member[:, 2] = n2 - member[:, 2]
                b["member"] = member.tolist()
    merged = copy.deepcopy(Bi)
    tree = types.SimpleNamespace(Bi=Bi)
    ns["grade"](tree)
    codes = [(str(g["index"]), str(g["fatherindex"])) for g in tree.Bi_g]
    # airway_parse: cd, first writer wins
    cd = np.zeros(label.shape, dtype=np.int32)
    claimed_twice = False
    for k, b in enumerate(Bi, start=1):
        vox = [b["start"]] + list(b["member"]) + ([b["end"]] if "end" in b else [])
        for p in vox:
            if cd[p[0], p[1], p[2]] == 0:
                cd[p[0], p[1], p[2]] = k
            elif cd[p[0], p[1], p[2]] != k:
                claimed_twice = True
    skeleton_parse = (cd != 0).astype(np.int32)
    parsing = ns["tree_parsing_func"](skeleton_parse, label, cd)
    flags.update(order=order, mainpart=int(mmm), smoothed=bool(B.shape != B0.shape or (B != B0).any()), claimed_twice=claimed_twice,
                 branches=(len(table1), len(merged)))
    rec.update(order=np.array(order), label_trans=LT.astype(np.uint8), skeleton=skel.astype(np.uint8), B0=B0.astype(np.int64),
               B=np.asarray(B).astype(np.int64), basev=np.asarray(basev, np.float64), mainpart=np.array(int(mmm)),
               codes=np.array([c for c, _ in codes]), father_codes=np.array([f for _, f in codes]),
               cd=cd.astype(np.int16), parsing=parsing.astype(np.int16))
    for name, table in (("table0", table0), ("table1", table1), ("merged", merged)):
        for k, v in flatten(table).items():
            rec[f"{name}_{k}"] = v
    assert len(merged) >= 3 and cd.max() < 32767
    return rec, flags


def tree_volume(spurs, flip):
    """40 x 72 x 150: a trunk (r^2 = 30) from z = 6 to 67 and three generations of forks; optionally four short spurs (r^2 = 3)
    along the trunk; optionally mirrored along axis 2."""
    import skeleton_oracle as so
    v = np.zeros((40, 72, 150), np.uint8)
    stamps = [((20, 36, 6), (20, 36, 67), 30),
              ((20, 36, 67), (20, 20, 97), 12), ((20, 36, 67), (20, 52, 99), 12),
              ((20, 20, 97), (12, 12, 122), 6), ((20, 20, 97), (27, 24, 124), 6),
              ((20, 52, 99), (13, 48, 125), 6), ((20, 52, 99), (28, 61, 123), 6),
              ((12, 12, 122), (6, 7, 144), 3), ((12, 12, 122), (16, 16, 145), 3),
              ((27, 24, 124), (23, 29, 146), 3), ((27, 24, 124), (33, 20, 144), 3),
              ((13, 48, 125), (8, 44, 145), 3), ((13, 48, 125), (17, 53, 146), 3),
              ((28, 61, 123), (24, 66, 144), 3), ((28, 61, 123), (34, 57, 145), 3)]
    if spurs:
        stamps += [((20, 36, 18), (20, 47, 20), 3), ((20, 36, 30), (20, 25, 32), 3), ((20, 36, 42), (31, 36, 44), 3),
                   ((20, 36, 54), (9, 36, 56), 3)]
    for a, b, r2 in stamps:
        so.stamp(v, a, b, r2)
    return v[:, :, ::-1].copy() if flip else v


def tripod_volume(arm_r2):
    """24 x 26 x 70: three arms from an apex at low axis-2 indices, five branches beyond them and two one-voxel twigs of 5 voxels."""
    import skeleton_oracle as so
    v = np.zeros((24, 26, 70), np.uint8)
    ends = [(5, 6, 26), (19, 6, 27), (12, 22, 28)]
    for e in ends:
        so.stamp(v, (12, 13, 3), e, arm_r2)
    for a, b in ((ends[0], (3, 4, 60)), (ends[0], (9, 10, 62)), (ends[1], (20, 4, 64)), (ends[1], (16, 11, 58)), (ends[2], (12, 22, 66))):
        so.stamp(v, a, b, 2)
    so.stamp(v, (12, 22, 45), (17, 22, 46), 0)
    so.stamp(v, (20, 4, 50), (15, 4, 51), 0)
    return v


def star_skeleton():
    """A hand-drawn skeleton whose first voxel has three ways on: three arms of 10 voxels, each forking into two of 8."""
    pts = [(5, 5, 0)]
    for d0, d1 in ((-1, -1), (1, -1), (0, 1)):
        arm = [(5 + d0, 5 + d1, 1)]
        for z in range(2, 11):
            arm.append((5 + 3 * d0, 5 + 3 * d1, z))
        arm[1:3] = [(5 + 2 * d0, 5 + 2 * d1, 2), (5 + 3 * d0, 5 + 3 * d1, 3)]
        pts += arm
        tip = arm[-1]
        for s in (-1, 1):
            pts += [(tip[0] + s * min(k, 3), tip[1], tip[2] + k) for k in range(1, 9)]
    return np.array(sorted(set(pts), key=lambda p: p[2]), dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (ours_skel_parse.py, ske_and_parse.py)")
    args = ap.parse_args()
    ns = reference_functions(args.reference)
    cases = [tree_volume(False, False), tree_volume(True, True), tripod_volume(1), tripod_volume(2)]
    data, allflags = {}, []
    for ci, label in enumerate(cases):
        rec, flags = run_reference(ns, label)
        print(f"case{ci}: shape {label.shape} skeleton {int(rec['skeleton'].sum())} {flags}")
        allflags.append(flags)
        for k, v in rec.items():
            data[f"case{ci}_{k}"] = v
    # the NaN path of compute_base_vector: two slabs with empty slices between them
    nan_vol = np.zeros((9, 10, 41), np.uint8)
    nan_vol[2:6, 3:8, 0:3] = 1
    nan_vol[3:7, 2:5, 38:41] = 1
    for order in (0, 1):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bv = ns["compute_base_vector"](nan_vol, order)
            mmm = ns["find_mainpart_index"](int(data["case0_B0"][0, 2]), run_tables(data, "case0_table0"), bv)
        assert np.isnan(bv).any() and mmm == 0
        data[f"nan_basev{order}"] = np.asarray(bv, np.float64)
    data["nan_volume"] = nan_vol
    # a multi-way start with three branches, at the functions: subsection, merging, grade on a hand-drawn skeleton
    star = star_skeleton()
    table = ns["subsection"](star.copy(), debug=1)
    star_multiway = max(sum(tuple(b["start"]) == s for b in table) for s in {tuple(b["start"]) for b in table})
    data["star_B"] = star
    for k, v in flatten(copy.deepcopy(table)).items():
        data[f"star_table_{k}"] = v
    merged = ns["merging"](table, 5)
    for k, v in flatten(copy.deepcopy(merged)).items():
        data[f"star_merged_{k}"] = v
    tree = types.SimpleNamespace(Bi=merged)
    ns["grade"](tree)
    data["star_codes"] = np.array([str(g["index"]) for g in tree.Bi_g])
    data["star_father_codes"] = np.array([str(g["fatherindex"]) for g in tree.Bi_g])
    print("star: branches", len(table), "->", len(merged), "multiway", star_multiway)
    assert {f["order"] for f in allflags} == {0, 1}
    assert any(f["mainpart"] > 1 and f["smoothed"] for f in allflags)
    assert any(f["leaf_cut"] and f["single_cut"] for f in allflags)
    assert star_multiway > 2 and any(f["multiway"] > 1 for f in allflags)
    assert any(f["claimed_twice"] for f in allflags)
    assert any(f["ties"] for f in allflags)
    assert any(any(n % 64 for n in c.shape) for c in cases) and any(c.shape[2] > 128 for c in cases)
    data["ncase"] = np.array(len(cases))
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


def run_tables(data, prefix):
    """A flattened table of ``data`` back as the reference's list of dicts."""
    out, at = [], 0
    for i in range(len(data[f"{prefix}_index"])):
        k = int(data[f"{prefix}_member_count"][i])
        b = {"index": int(data[f"{prefix}_index"][i]), "start": data[f"{prefix}_start"][i].tolist(),
             "member": data[f"{prefix}_members"][at:at + k].tolist(), "fatherindex": int(data[f"{prefix}_fatherindex"][i])}
        if data[f"{prefix}_has_end"][i]:
            b["end"] = data[f"{prefix}_end"][i].tolist()
        out.append(b)
        at += k
    return out


if __name__ == "__main__":
    main()
