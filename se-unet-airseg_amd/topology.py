"""The graph stage of ``airway_parse``: the reference's own branch parser (ours_skel_parse.py:30-481, :569-646 and the glue of
ske_and_parse.py:20-59) restated on the host with numpy only.  It runs on the few thousand voxels of a skeleton, so it needs no
GPU and is importable and testable without one; the dense stages around it are HIP kernels (prep.airway_parse, DESIGN.md
section 3g).

A branch is a dict ``{"index", "fatherindex", "start", "member", ["end"]}`` with coordinates as tuples of Python ints.  All
functions are pure: they return new tables and leave their arguments alone.  Two stated choices: every sort is
stable, and where the reference raises some exception, ``ValueError`` naming the stage is raised here."""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

Point = Tuple[int, int, int]
Branch = Dict[str, object]


def _neighbour_order() -> Tuple[Point, ...]:
    """The 26 offsets in the visiting order that decides the results: the 8 with d2 = 0, then the 9 with d2 = -1, then the 9
    with d2 = +1, each group in raster order of (d0, d1)."""
    out = []
    for d2 in (0, -1, 1):
        for d0 in (-1, 0, 1):
            for d1 in (-1, 0, 1):
                if (d0, d1, d2) != (0, 0, 0):
                    out.append((d0, d1, d2))
    return tuple(out)


NEIGHBOURS = _neighbour_order()


def _fail(stage: str, why: str):
    raise ValueError(f"airway_parse: {stage}: {why}")


# ---- orientation (ske_and_parse.py:21-37) ----------------------------------------------------------------------------------

def orientation_slices(minz: int, maxz: int) -> Tuple[int, int]:
    """The two axis-2 slices whose largest 8-connected component decides the orientation: at 0.2 and at 0.8 of the extent."""
    cha = maxz - minz
    return int(0.2 * cha + minz), int(0.8 * cha + minz)


def orientation(size_at_02: int, size_at_08: int) -> int:
    """0 when the slice at 0.2 holds the larger component (the trachea lies at low axis-2 indices), else 1."""
    return 0 if size_at_02 > size_at_08 else 1


# ---- skeleton coordinates (Topology_Tree.sub, ours_skel_parse.py:581-589) -------------------------------------------------

def sorted_skeleton(coords, order: int, n2: int) -> np.ndarray:
    """Skeleton coordinates (raster order, (m, 3)) sorted by their axis-2 coordinate with a stable sort; for ``order == 1`` the
    third coordinate becomes ``n2 - z`` after sorting."""
    B = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    if B.shape[0] == 0:
        _fail("skeleton", "the skeleton is empty")
    B = B[np.argsort(B[:, 2], kind="stable")].copy()
    if order == 1:
        B[:, 2] = n2 - B[:, 2]
    return B


# ---- subsection (ours_skel_parse.py:30-164 with debug = 1) ------------------------------------------------------------------

def subsection(B) -> List[Branch]:
    """Cut the skeleton ``B`` ((m, 3) integer rows) into branches by a breadth-first walk from the first row with the lowest
    third coordinate.  Kept as the reference has them: a voxel ends a branch when at least 3 skeleton voxels lie around it,
    visited or not; the sibling branches of a multi-way start share the running member list; branch numbers at such a start
    can repeat."""
    rows = [tuple(int(v) for v in r) for r in np.asarray(B).reshape(-1, 3)]
    if not rows:
        _fail("subsection", "the skeleton is empty")
    skeleton = set(rows)
    lowest = min(r[2] for r in rows)
    seed = next(r for r in rows if r[2] == lowest)
    visited = {seed}
    starts: List[Tuple[Point, int]] = [(seed, 0)]          # (voxel, number of the branch that found it)
    table: List[Branch] = []
    number = 0

    def around(p):
        return [(p[0] + d[0], p[1] + d[1], p[2] + d[2]) for d in NEIGHBOURS]

    def walk(fifo, branch, member):
        """Follow ``fifo`` until a junction (-> branch["end"], its unvisited neighbours become starts) or until it runs dry."""
        while fifo:
            p = fifo[0]
            count, fresh = 0, []
            for q in around(p):
                if q in skeleton:
                    count += 1
                    if q not in visited:
                        fifo.append(q)
                        fresh.append(q)
            visited.add(p)
            if count >= 3:
                branch["end"] = p
                starts.extend((q, number) for q in fresh)
                visited.update(fresh)
                return
            member.append(p)
            del fifo[0]

    while starts:
        origin, father = starts[0]
        number += 1
        links = [q for q in around(origin) if q in skeleton and q not in visited]
        member: List[Point] = []
        if len(links) > 1:
            for l in range(1, len(links)):                     # every link but the first, in order; the first goes last
                number += l - 1
                branch = {"index": number, "start": origin}
                walk([links[l]], branch, member)
                branch["member"] = list(member)                # the siblings share the running list
                branch["fatherindex"] = father
                table.append(branch)
            links = links[:1]
            number += 1
            member = []
        branch = {"index": number, "start": origin}
        walk(links, branch, member)
        branch["member"] = list(member)
        branch["fatherindex"] = father
        table.append(branch)
        del starts[0]
    return table


# ---- main part (ours_skel_parse.py:166-245) ----------------------------------------------------------------------------------

def base_vector_slices(minz: int, maxz: int, order: int) -> Tuple[int, int]:
    """The two axis-2 slices of LABEL_TRANS whose centroids span the base vector."""
    cha = maxz - minz
    if order == 1:
        return int(maxz - 0.1 * cha), int(0.6 * cha + minz)
    return int(minz + 0.1 * cha), int(0.4 * cha + minz)


def slice_centroid(count: int, sum0: int, sum1: int) -> Tuple[float, float]:
    """numpy's mean of the coordinates of a slice from the exact integer sums; an empty slice gives NaN."""
    if count == 0:
        return math.nan, math.nan
    return float(np.float64(sum0) / np.float64(count)), float(np.float64(sum1) / np.float64(count))


def base_vector(minz: int, maxz: int, order: int, moments: Callable[[int], Sequence[int]]) -> np.ndarray:
    """``compute_base_vector``: from the centroid of slice 1 to the centroid of slice 2 (``base_vector_slices``); ``moments(k)``
    returns (count, sum of i0, sum of i1) of slice k of LABEL_TRANS."""
    k1, k2 = base_vector_slices(minz, maxz, order)
    c1, c2 = slice_centroid(*moments(k1)), slice_centroid(*moments(k2))
    dz = k1 - k2 if order == 1 else k2 - k1
    return np.array([c2[0] - c1[0], c2[1] - c1[1], dz])


def cosine(a, b) -> float:
    return np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b))


def find_mainpart_index(first_z: int, table: Sequence[Branch], basev) -> int:
    """Index of the branch at which the main airway ends: among the first 21 branches with more than 12 members (stopping at one
    with more than ``first_z / 3.6``), the first whose cosine to ``basev`` falls below 0.93 after one above 0.928 was seen.  0
    when there is none; NaN cosines (an empty slice behind ``basev``) compare false everywhere and give 0."""
    main = []
    for i, b in enumerate(table):
        m = b["member"]
        if i > 20:
            break
        if len(m) == 0:
            continue
        if len(m) > first_z / 3.6:
            break
        if len(m) > 12:
            main.append((i, cosine(basev, np.array(m[-1]) - np.array(b["start"]))))
    seen = False
    for i, cos in main:
        if cos < 0.928 and not seen:
            continue
        if cos > 0.928:
            seen = True
        if cos < 0.93 and seen:
            return i
    return 0


# ---- smoothing of the main airway (ours_skel_parse.py:247-386) ---------------------------------------------------------------

def interp_linear(knots_x, knots_y, n: int) -> np.ndarray:
    """scipy's linear ``interp1d`` (extrapolating) through (knots_x, knots_y) at the abscissae 0 .. n - 1, in float64 and in its
    form ``slope * (x - x_lo) + y_lo``; at a knot the segment on its left is used."""
    x = np.asarray(knots_x)
    y = np.asarray(knots_y).astype(np.float64)
    xs = np.arange(n, dtype=np.float64)
    hi = np.clip(np.searchsorted(x, xs), 1, len(x) - 1).astype(int)
    lo = hi - 1
    slope = (y[hi] - y[lo]) / (x[hi] - x[lo])
    return slope * (xs - x[lo]) + y[lo]


def _step_towards(prev: int, v: int) -> int:
    return prev + (1 if v > prev else -1) if abs(v - prev) > 1 else v


def smooth_points(points) -> np.ndarray:
    """Replace a polyline by the rounded piecewise-linear curve through three or four of its points: knots every ``n // 3`` rows
    plus the last row (the knot before it dropped when closer than 5), ``np.round`` (half to even), each coordinate held within
    1 of the row before; then a stable sort by the third coordinate, one row per value of it, and the same hold from the far
    end.  Returns the rows in ascending third coordinate."""
    P = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    n = len(P)
    if n < 3:
        _fail("smoothing", f"{n} main-airway points (at least 3 are needed)")
    knots = np.append(np.arange(0, n, n // 3), n - 1)
    if abs(int(knots[-2]) - int(knots[-1])) < 5:
        knots = np.delete(knots, -2)
    curve = np.stack([interp_linear(knots, P[knots, a], n) for a in range(3)], axis=1)
    rounded = np.round(curve).astype(np.int64)
    held = [tuple(int(v) for v in rounded[0])]
    for r in rounded[1:]:
        held.append(tuple(_step_towards(held[-1][a], int(r[a])) for a in range(3)))
    held.sort(key=lambda p: p[2])                                   # list.sort is stable
    unique = [p for k, p in enumerate(held) if k == 0 or p[2] != held[k - 1][2]]
    unique.reverse()
    final = [unique[0]]
    for p in unique[1:]:
        final.append(tuple(_step_towards(final[-1][a], p[a]) for a in range(3)))
    final.reverse()
    return np.array(final, dtype=np.int64).reshape(-1, 3)


def process_mainairway_points(B, table: Sequence[Branch], mainpart: int) -> np.ndarray:
    """The skeleton with the voxels of the first ``mainpart`` branches replaced by their smoothed curve: those voxels, without
    repeats, ordered from the end of ``B`` to its start; the first ones beyond the curve's length leave ``B``; the others take the
    curve's rows one for one."""
    B = np.asarray(B, dtype=np.int64).reshape(-1, 3)
    rows = [tuple(int(v) for v in r) for r in B]
    position = {r: i for i, r in enumerate(reversed(rows))}
    main = set()
    for b in table[:mainpart]:
        main.add(tuple(b["start"]))
        main.update(tuple(p) for p in b["member"])
        if "end" in b:
            main.add(tuple(b["end"]))
    main = sorted(main, key=lambda r: position[r])
    curve = smooth_points(np.array(main, dtype=np.int64))
    dropped = set(main[:len(main) - len(curve)])
    kept = main[len(main) - len(curve):]
    out = np.array([r for r in rows if r not in dropped], dtype=np.int64).reshape(-1, 3)
    where = {}
    for i, r in enumerate(map(tuple, out.tolist())):
        where.setdefault(r, []).append(i)
    for r, new in zip(kept, curve):
        for i in where[r]:
            out[i] = new
    return out


# ---- merging (ours_skel_parse.py:388-481) ------------------------------------------------------------------------------------

def branch_voxels(b: Branch) -> List[Point]:
    """start + member + end."""
    return [b["start"]] + list(b["member"]) + ([b["end"]] if "end" in b else [])


def merging(table: Sequence[Branch], len_thre: int) -> List[Branch]:
    """Remove short branches.  First, a branch of at most ``len_thre`` voxels goes: a leaf is dropped, otherwise every branch whose
    father number equals its POSITION + 1 takes over its father, its start and its voxels.  Then a branch with exactly one child
    (the first such father number is left out, as the reference leaves it) absorbs that child."""
    T = [dict(b, member=list(b["member"])) for b in table]
    cut = set()
    for i, bi in enumerate(T):
        if len(branch_voxels(bi)) > len_thre:
            continue
        sons = 0
        for bj in T[i + 1:]:
            if bj["fatherindex"] != i + 1:
                continue
            sons += 1
            bj["fatherindex"] = bi["fatherindex"]
            bj["member"] = branch_voxels(bi)[1:] + [bj["start"]] + bj["member"]
            bj["start"] = bi["start"]
        cut.add(i)
    T = [b for i, b in enumerate(T) if i not in cut]
    if not T:
        _fail("merging", "no branch is left after the short branches were removed")

    size = T[-1]["index"]
    children = np.zeros(size, dtype=np.int64)
    for b in T:
        f = b["fatherindex"]
        if not 0 <= f < size:
            _fail("merging", f"father number {f} is outside the child table of {size} entries (child_num overflow)")
        children[f] += 1
    single = [int(s) for s in np.flatnonzero(children == 1)][1:]
    parents = [i for s in single for i, b in enumerate(T) if b["index"] == s]
    absorbed = set()
    pairs = []
    for pi in reversed(parents):
        pair = (0, 0)
        parent = T[pi]
        for i in range(len(T) - 1, -1, -1):
            child = T[i]
            if child["fatherindex"] != parent["index"]:
                continue
            if "end" not in parent:
                _fail("merging", f"branch {parent['index']} has a child but no end voxel")
            pair = (child["fatherindex"], child["index"])
            absorbed.add(i)
            chain = [parent["end"], child["start"]] + list(child["member"])
            if "end" in child:
                parent["end"] = child["end"]
            else:
                parent["end"] = chain.pop()
            parent["member"] = parent["member"] + chain
        pairs.append(pair)
    for father, child in pairs:                                     # (pairs is already in the reference's reversed order)
        for b in reversed(T):
            if b["fatherindex"] == child:
                b["fatherindex"] = father
    return [b for i, b in enumerate(T) if i not in absorbed]


def flip_back(table: Sequence[Branch], n2: int) -> List[Branch]:
    """``merge()`` for order 1: the third coordinate of every voxel becomes ``n2 - z`` again."""
    def f(p):
        return (p[0], p[1], n2 - p[2])
    out = []
    for b in table:
        c = dict(b, start=f(b["start"]), member=[f(p) for p in b["member"]])
        if "end" in b:
            c["end"] = f(b["end"])
        out.append(c)
    return out


# ---- grade (ours_skel_parse.py:621-646) ---------------------------------------------------------------------------------------

def grade(table: Sequence[Branch]) -> List[Tuple[str, str]]:
    """The code string of every branch and of its father: '0' for the first; '00' / '01' for the next two, '01' going to the one
    whose start lies further along axis 1; from the fourth on the father's code plus the running count of its children.  A
    father number no branch carries leaves the search at the last branch with the code of the previous round, as the reference's
    loop does."""
    n = len(table)
    if n < 3:
        _fail("grade", f"{n} branches after merging (the first three are addressed by position)")
    code = [None] * n
    father = [None] * n
    code[0], father[0] = "0", "-1"
    second_is_left = table[1]["start"][1] > table[2]["start"][1]
    code[1], code[2] = ("01", "00") if second_is_left else ("00", "01")
    father[1] = father[2] = "0"
    used = [0] * n
    string: Optional[str] = None
    for i in range(3, n):
        g = n - 1
        for k in range(n):
            if table[k]["index"] == table[i]["fatherindex"]:
                g = k
                string = code[k] + str(used[k])
                break
        if string is None:
            _fail("grade", f"branch {table[i]['index']}: no branch carries its father number {table[i]['fatherindex']}")
        used[g] += 1
        code[i] = string
        father[i] = code[g]
    return list(zip(code, father))


# ---- cd (ske_and_parse.py:48-59) -----------------------------------------------------------------------------------------------

def branch_labels(table: Sequence[Branch], shape: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """``cd`` as (raster indices int64, values int32): branch k of the table (1-based, table order) writes k at start + member +
    end, and the first writer of a voxel wins, so every index appears once."""
    n0, n1, n2 = (int(v) for v in shape)
    first: Dict[int, int] = {}
    for k, b in enumerate(table, start=1):
        for p in branch_voxels(b):
            if not (0 <= p[0] < n0 and 0 <= p[1] < n1 and 0 <= p[2] < n2):
                _fail("cd", f"voxel {tuple(p)} of branch {k} lies outside the volume {(n0, n1, n2)}")
            first.setdefault((p[0] * n1 + p[1]) * n2 + p[2], k)
    lin = np.fromiter(first.keys(), dtype=np.int64, count=len(first))
    val = np.fromiter(first.values(), dtype=np.int32, count=len(first))
    return lin, val


# ---- the whole stage ------------------------------------------------------------------------------------------------------------

def graph_stage(coords, shape: Sequence[int], order: int, z_extent: Tuple[int, int], moments: Callable[[int], Sequence[int]],
                merge_t: int = 5, trace: Optional[dict] = None):
    """From the skeleton of LABEL_TRANS to the merged branch table: ``coords`` its voxels in raster order, ``z_extent`` the
    (min, max) axis-2 coordinate of LABEL_TRANS, ``moments(k)`` the (count, sum i0, sum i1) of its slice k.  Returns
    ``(table, codes)``; ``trace`` (a dict) receives the intermediate results."""
    n2 = int(shape[2])
    B0 = sorted_skeleton(coords, order, n2)
    table0 = subsection(B0)
    basev = base_vector(int(z_extent[0]), int(z_extent[1]), order, moments)
    mainpart = find_mainpart_index(int(B0[0, 2]), table0, basev)
    if mainpart > 1:
        B = process_mainairway_points(B0, table0, mainpart)
        table1 = subsection(B)
    else:
        B, table1 = B0, table0
    merged = merging(table1, merge_t)
    if order == 1:
        merged = flip_back(merged, n2)
    codes = grade(merged)
    if trace is not None:
        trace.update(B0=B0, table0=table0, basev=basev, mainpart=mainpart, B=B, table1=table1, merged=merged, codes=codes)
    return merged, codes


# ---- flat form of a table (fixtures, tests) -----------------------------------------------------------------------------------

def flatten(table: Sequence[Branch]) -> Dict[str, np.ndarray]:
    """A branch table as arrays: index, fatherindex, start (n, 3), has_end, end (n, 3, zeros where absent), member_count and the
    members of all branches back to back (m, 3)."""
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


def unflatten(flat: Dict[str, np.ndarray]) -> List[Branch]:
    out, at = [], 0
    for i in range(len(flat["index"])):
        k = int(flat["member_count"][i])
        b = {"index": int(flat["index"][i]), "start": tuple(int(v) for v in flat["start"][i]),
             "member": [tuple(int(v) for v in p) for p in flat["members"][at:at + k]], "fatherindex": int(flat["fatherindex"][i])}
        if flat["has_end"][i]:
            b["end"] = tuple(int(v) for v in flat["end"][i])
        out.append(b)
        at += k
    return out
