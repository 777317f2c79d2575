"""The ATM'22 airway tree parser stated in numpy / scipy: the travelling oracle of tests/test_parse_gpu.py.

What it states is atm22_skel_parse.py:83-260 as driven by tree_parsing.py:114-159 (meshes and pictures left out), in this
project's own words.  tests/test_parse_host.py pins it to the reference: it reproduces every array of
tests/golden/parse_known.npz, which scripts/make_golden_parse.py recorded from the reference's own functions.  Unlike
``seunet_amd.prep.tree_parsing`` it takes the voxel counts and the adjacency from the volume again in every refinement round, as
the reference does, so the two are independent statements of the same result.  Plain rather than fast.
"""
import numpy as np
from scipy import ndimage

CUBE = np.ones((3, 3, 3), dtype=bool)
CROSS = ndimage.generate_binary_structure(3, 1)


def skeleton_parsing(skeleton, min_voxels=5, mode="reflect"):
    """-> (skeleton_parse uint8, cd int32, num).  A skeleton voxel with more than two neighbours in its 3x3x3 block, counted
    with scipy's `mode` at the border ('reflect': a voxel on a face sees itself and its in-face neighbours again), is a branch
    point and goes; the rest is labelled with 26-connectivity; components under `min_voxels` voxels go; what is left is
    labelled again, so the numbers are consecutive in raster order of each component's first voxel."""
    s = (np.asarray(skeleton) != 0)
    total = ndimage.convolve(s.astype(np.float32), CUBE.astype(np.float32), mode=mode)
    keep = s & ~(total > 3)
    cd, num = ndimage.label(keep, structure=CUBE)
    sizes = np.bincount(cd.ravel(), minlength=num + 1)
    small = sizes < min_voxels
    small[0] = False
    keep = keep & ~small[cd]
    cd, num = ndimage.label(keep, structure=CUBE)
    return keep.astype(np.uint8), cd.astype(np.int32), int(num)


def tree_parsing_func(skeleton_parse, label, cd):
    """Every label voxel takes the number of the nearest skeleton_parse voxel (scipy's feature transform decides ties)."""
    idx = ndimage.distance_transform_edt(np.asarray(skeleton_parse) == 0, return_distances=False, return_indices=True)
    return (np.asarray(cd)[idx[0], idx[1], idx[2]] * (np.asarray(label) != 0)).astype(np.int32)


def label_counts(parsing, num):
    return np.bincount(parsing.ravel(), minlength=num + 1)[1:num + 1].astype(np.int64)


def adjacent_map(parsing, num):
    """ad[i, j] = 1 iff a voxel of label j + 1 lies in the 6-neighbourhood shell of label i + 1."""
    ad = np.zeros((num, num), dtype=np.uint8)
    for i in range(num):
        own = parsing == i + 1
        if not own.any():
            continue
        shell = ndimage.binary_dilation(own, structure=CROSS) & ~own
        for v in np.unique(parsing[shell]):
            if v > 0:
                ad[i, v - 1] = 1
    return ad


def parent_children_map(ad, trachea, num):
    """Breadth first from the trachea (0-based).  A level is emptied from its end; children are visited in ascending order;
    an unvisited child takes the current node as parent and its generation + 1; a visited one takes it as a further parent
    when it lies exactly one generation below.  The generation is uint8 and wraps, as in the reference."""
    parent = np.zeros((num, num), dtype=np.uint8)
    children = np.zeros((num, num), dtype=np.uint8)
    generation = np.zeros(num, dtype=np.uint8)
    parent[trachea, trachea] = 1
    level = [trachea]
    while level:
        todo, level = level, []
        while todo:
            cur = todo.pop()
            for child in np.where(ad[cur] > 0)[0]:
                if parent[child].sum() == 0:
                    parent[child, cur] = 1
                    children[cur, child] = 1
                    generation[child] = generation[cur] + 1
                    level.append(child)
                elif generation[cur] + 1 == generation[child]:
                    parent[child, cur] = 1
                    children[cur, child] = 1
    return parent, children, generation


def merge_sweep(parent, children, vol):
    """One merge sweep on `vol`, in place -> the deleted labels (0-based) in order.  First every node with several parents
    fuses them into the first one; then every node with exactly one child swallows it, unless either was deleted already."""
    deleted = []
    for node in np.where(parent.sum(axis=1) > 1)[0]:
        ps = np.where(parent[node] > 0)[0]
        for p in ps[1:]:
            vol[vol == p + 1] = ps[0] + 1
            if p not in deleted:
                deleted.append(p)
    for node in np.where(children.sum(axis=1) == 1)[0]:
        if node in deleted:
            continue
        child = np.where(children[node] == 1)[0][0]
        if child not in deleted:
            vol[vol == child + 1] = node + 1
            deleted.append(child)
    return deleted


def refinement_round(vol, num):
    """One turn of the loop on `vol` (in place) -> (changed, new num, trachea 1-based, counts, ad)."""
    counts = label_counts(vol, num)
    trachea = int(np.argsort(counts.astype(np.float64))[-1])
    ad = adjacent_map(vol, num)
    parent, children, _ = parent_children_map(ad, trachea, num)
    if not merge_sweep(parent, children, vol):           # the test of the loop merges in place ...
        return False, num, trachea + 1, counts, ad
    deleted = merge_sweep(parent, children, vol)          # ... and the body merges again on the merged volume
    gone = np.array(deleted)
    for i in range(num):                                  # then the numbers close up, in place and in ascending order
        if i not in deleted:
            vol[vol == i + 1] = i + 1 - int((gone < i).sum())
    return True, num - len(deleted), trachea + 1, counts, ad


def tree_parsing(label, skeleton, refine=True):
    """-> dict: skeleton_parse, cd, num0, parsing0 (before the loop), counts0 / ad0 / trachea0 (first round), rounds, parsing,
    num (after the loop; = parsing0 / num0 with refine=False)."""
    skeleton_parse, cd, num = skeleton_parsing(skeleton)
    vol = tree_parsing_func(skeleton_parse, label, cd)
    out = {"skeleton_parse": skeleton_parse, "cd": cd, "num0": num, "parsing0": vol.copy(), "rounds": 0}
    first = True
    while refine:
        changed, num, trachea, counts, ad = refinement_round(vol, num)
        if first:
            out["counts0"], out["ad0"], out["trachea0"] = counts, ad, trachea
            first = False
        if not changed:
            break
        out["rounds"] += 1
    out["parsing"], out["num"] = vol, num
    return out
