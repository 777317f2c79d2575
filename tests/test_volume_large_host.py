"""That the cases of tests/volume_large_cases.py reach what they name, without a GPU ("Tests past 2^20
elements"):

* the constants the cases restate are the ones in csrc/bitvol.h, csrc/bitvol.hip and csrc/volume.h, read as text -- whoever changes
  a block size is told here that the cases must move;
* every case has the word count, the number of block totals and the number of chunks of the top scan that its line states;
* from the oracles' output, the quantity each scan runs over is non-zero in every chunk -- before and after every chunk border --
  and, for ``ends`` and ``gap``, zero over the run of blocks the case is named for.  A case that fails this is a wrong case;
* the label case has more than 2^22 vertices and faces (more than 2^20 histogram bins in both sorts) and two radix passes;
* scipy's transform with sampling, which stands in for tests/surface_oracle.py at this size, equals tests/edt_sampling_oracle.py
  bit for bit on a 6 x 7 x 70 mask."""
import os
import re

import numpy as np
import pytest

import edt_sampling_oracle as eo
import mesh_oracle as mo
import surface_oracle as so
import volume_large_cases as vc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "se-unet-airseg_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_restated_constants_are_the_sources():
    assert re.findall(r"constexpr int kScanBlock = (\d+);", source("bitvol.h")) == [str(vc.SCAN_BLOCK)]
    assert re.findall(r"constexpr int kSortBlock = (\d+);", source("volume.h")) == [str(vc.SORT_BLOCK)]
    hip = source("bitvol.hip")
    assert re.findall(r"scan_top_kernel<<<1, (\d+), 0, s>>>", hip) == [str(vc.TOP_THREADS)]
    top = hip[hip.index("scan_top_kernel("):hip.index("scan_add_kernel(")]
    assert re.findall(r"for \(long long c = 0; c < nb; c \+= (\d+)\)", top) == [str(vc.TOP_THREADS)]
    assert re.findall(r"__shared__ u64 sh\[2\]\[(\d+)\];", top) == [str(vc.TOP_THREADS)]
    assert re.findall(r"if \(tid == (\d+)\) carry = before", top) == [str(vc.TOP_THREADS - 1)]
    assert vc.CHUNK == 1 << 20
    # one scan block per workgroup of 256 threads x 4 elements
    assert re.findall(r"scan_block_kernel<<<\(unsigned\)nb, (\d+), 0, s>>>", hip) == [str(vc.SCAN_BLOCK // 4)]


@pytest.mark.parametrize("name", list(vc.CASES))
def test_words_block_totals_and_chunks(name):
    shape, zero, words, totals, trips = vc.CASES[name]
    assert shape[2] == 2 and vc.word_count(shape) == shape[0] * shape[1] == words
    assert vc.block_totals(words) == totals and vc.chunks(words) == trips
    assert len(vc.chunk_borders(words)) == trips - 1
    assert max(shape) <= 32767 and shape[0] * shape[1] * shape[2] < 2 ** 31          # kEdtMaxExtent, volume_check
    if name == "exact":
        assert words == vc.CHUNK                                   # thread 1023 holds the last block total, and no chunk follows
    if name == "one_more":
        assert words - vc.CHUNK == vc.SCAN_BLOCK                   # the second chunk is one full block
    if name == "ragged":
        assert words - vc.CHUNK == vc.SCAN_BLOCK + 1021 and words % vc.SCAN_BLOCK == 1021 and words % 4 == 1
    if zero is not None:
        assert 0 < zero[0] < zero[1] < shape[0]


def per_chunk(counts):
    """Sum of a per-element count over each chunk of the top scan."""
    n = len(counts)
    return [int(counts[c * vc.CHUNK:min((c + 1) * vc.CHUNK, n)].sum()) for c in range(vc.chunks(n))]


def per_block(counts):
    pad = np.zeros(vc.block_totals(len(counts)) * vc.SCAN_BLOCK, np.int64)
    pad[:len(counts)] = counts
    return pad.reshape(-1, vc.SCAN_BLOCK).sum(axis=1)


def zero_run(name, counts, first_plane, last_plane):
    """The counts of the words of planes first_plane .. last_plane - 1 are zero, and those of the planes on either side are not."""
    shape = vc.CASES[name][0]
    lo, hi = first_plane * shape[1], last_plane * shape[1]
    assert not counts[lo:hi].any()
    assert counts[lo - shape[1]:lo].any() and counts[hi:hi + shape[1]].any()
    return lo, hi


@pytest.mark.parametrize("name", vc.MESH_CASES)
def test_the_mesh_counts_are_non_zero_in_every_chunk(name):
    shape, zero, words, totals, trips = vc.CASES[name]
    v, verts, faces = vc.mesh(name)
    print(name, "V", len(verts), "F", len(faces))
    owner = np.floor(verts[:, 0]).astype(np.int64) * shape[1] + np.floor(verts[:, 1]).astype(np.int64)   # the word of the owning voxel
    assert np.all(np.diff(owner) >= 0)                                             # raster order
    vcnt = np.bincount(owner, minlength=words)
    assert vcnt.size == words and all(c > 0 for c in per_chunk(vcnt)), per_chunk(vcnt)
    assert per_block(vcnt)[-1] > 0                                                 # the last block total, thread (totals - 1) % 1024
    # The triangles per word, from the oracle's table: a row has one cell, counted at the word of its base voxel; the last row of
    # a plane and the last plane have none, so a chunk that lies in the last plane scans zero triangle counts.
    config = np.zeros((shape[0] - 1, shape[1] - 1), np.int64)
    for bit, d in enumerate(mo.CORNERS):
        config |= (v[d[0]:d[0] + shape[0] - 1, d[1]:d[1] + shape[1] - 1, d[2]] != 0).astype(np.int64) << bit
    fcnt = np.zeros(shape[:2], np.int64)
    fcnt[:-1, :-1] = mo.TRI_COUNT[config]
    fcnt = fcnt.reshape(-1)
    assert int(fcnt.sum()) == len(faces)
    cell_words = (shape[0] - 1) * shape[1]
    print(name, "vertices per chunk", per_chunk(vcnt), "triangles per chunk", per_chunk(fcnt))
    for c, n in enumerate(per_chunk(fcnt)):
        assert n > 0 or c * vc.CHUNK >= cell_words, (name, c)
    if name in ("ragged", "gap"):                                                  # the triangle scan carries into a chunk with cells
        assert per_chunk(fcnt)[1] > 0
    if name == "ends":                                                             # 896 zero block totals inside the first chunk
        lo, hi = zero_run(name, vcnt, 64, 960)
        assert hi < vc.CHUNK and not per_block(vcnt)[64:960].any() and per_chunk(vcnt)[1] > 0
    if name == "gap":                                                              # zero across the border
        lo, hi = zero_run(name, vcnt, 64, 1035)
        assert lo < vc.CHUNK - 900 * vc.SCAN_BLOCK and vc.CHUNK + 10 * vc.SCAN_BLOCK < hi
    if name == "one_more":
        assert (len(verts), len(faces)) == (2622237, 3355672)
        # the adjacency of this mesh: 2561 block totals, three chunks, in the scan of the list lengths and of the degrees
        assert vc.block_totals(len(verts)) == 2561 and vc.chunks(len(verts)) == 3
        used = np.bincount(faces.reshape(-1), minlength=len(verts))
        assert used.all() and all(c > 0 for c in per_chunk(used))


@pytest.mark.parametrize("name", vc.SURFACE_CASES)
def test_the_border_counts_are_non_zero_in_every_chunk(name):
    shape, zero, words, totals, trips = vc.CASES[name]
    a, b, ba, bb = vc.surface_masks(name)
    for which, border in (("a", ba), ("b", bb)):
        cnt = border.reshape(words, -1).sum(axis=1)
        print(name, which, "border voxels", int(cnt.sum()), "non-empty words per chunk", [int((cnt[c * vc.CHUNK:(c + 1) * vc.CHUNK] != 0).sum())
                                                                                       for c in range(trips)])
        assert all(c > 0 for c in per_chunk(cnt)) and per_block(cnt)[-1] > 0
        if name == "ends":
            lo, hi = zero_run(name, cnt, 64, 961)
            assert hi < vc.CHUNK and not per_block(cnt)[64:961].any()
        if name == "gap":
            lo, hi = zero_run(name, cnt, 64, 1036)
            assert lo < vc.CHUNK - 900 * vc.SCAN_BLOCK and vc.CHUNK + 10 * vc.SCAN_BLOCK < hi
        if name == "one_more" and which == "a":
            assert (int((cnt[:vc.CHUNK] != 0).sum()), int((cnt[vc.CHUNK:] != 0).sum())) == (786336, 780)
    if name == "one_more":
        assert (int(ba.sum()), int(bb.sum())) == (1049416, 1048858)


def test_the_label_case_has_more_than_2_to_the_20_bins_in_both_sorts():
    L, (verts, faces, vert_ptr, face_ptr) = vc.labels()
    V, F = len(verts), len(faces)
    print("V", V, "F", F, "bins", vc.sort_bins(V), vc.sort_bins(F))
    assert L.dtype == np.int32 and set(np.unique(L).tolist()) == {0, 1, vc.LABEL_NUM}
    assert V > 4194304 and F > 4194304 and vc.LABEL_NUM >= 256                       # two radix passes, both past one chunk
    assert (V, F) == (5187422, 6436289)
    assert vc.sort_bins(V) == 5066 * 256 > vc.CHUNK and vc.sort_bins(F) == 6286 * 256 > vc.CHUNK
    assert vc.chunks(vc.sort_bins(V)) == 2 and vc.chunks(vc.sort_bins(F)) == 2
    assert len(vert_ptr) == vc.LABEL_NUM + 1 and vert_ptr[[1, 299, 300]].tolist() == [2593637, 2593637, 5187422]
    assert 0 < face_ptr[1] == face_ptr[299] < face_ptr[300] == F
    # The labels 1 and 300 fill bins of the first chunk only (digits 1, 44 and 0, 1): their sorts scan past 2^20 bins, but what
    # they scan there is zero.  The renamed labellings put items on both sides of the border in every pass they run.
    for n in (V, F):
        for shift in (0, 8):
            assert all(last <= vc.CHUNK for _, last in vc.digit_bins(n, (1, vc.LABEL_NUM), shift))
        for which, shifts in (("two_passes", (0, 8)), ("one_pass", (0,))):
            top = vc.LABEL_TOPS[which]
            for shift in shifts:
                (first_lo, last_lo), (first_hi, last_hi) = vc.digit_bins(n, (1, top), shift)
                assert last_lo <= vc.CHUNK <= first_hi and last_hi == vc.sort_bins(n), (which, shift)
    assert vc.LABEL_TOPS["one_pass"] < 256 <= vc.LABEL_TOPS["two_passes"] <= 65535


def test_renaming_the_larger_label_only_changes_the_pointer_arrays():
    import mesh_label_oracle as lo
    L = lo.random_labels((5, 6, 7), 2, 0.9, 2)
    L[L == 2] = vc.LABEL_NUM
    res = lo.label_meshes(L)
    assert len(res[0]) and res[2][1] not in (0, len(res[0]))
    for top in (255, 700):
        want = lo.label_meshes(np.where(L == vc.LABEL_NUM, top, L))
        got = vc.relabel_result(res, top)
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want)), top
    want = lo.label_meshes(np.where(L == vc.LABEL_NUM, 0, L), 1)
    got = (res[0][:res[2][1]], res[1][:res[3][1]], res[2][:2], res[3][:2])
    assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))


def test_scipy_with_sampling_equals_the_edt_oracle():
    ndimage = pytest.importorskip("scipy.ndimage")
    border = so.border(vc.noise((6, 7, 70), 0.5, 670))
    assert border.any() and not border.all()
    want, _ = eo.edt((~border).astype(np.uint8), [float(v) for v in vc.SPACING])
    got = ndimage.distance_transform_edt(~border, sampling=[float(v) for v in vc.SPACING])
    assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64))
    assert np.unique(got).size > 5
