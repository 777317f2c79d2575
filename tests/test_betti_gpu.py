"""Component labelling, Euler number, Betti numbers and the Betti error on the GPU against tests/betti_oracle.py: every public call
of ``seunet_amd.components``, bit for bit, exact integer equality everywhere.  The cases and what makes each worth running are
asserted on the CPU in tests/test_betti_host.py."""
import numpy as np
import pytest
import torch

import betti_oracle as bo
from test_betti_host import NAMES, volume

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import seunet_amd
    seunet_amd._lib.load()
    return seunet_amd


def check_label(A, v, connectivity, sizes=(1, 2, 50)):
    """label with its count and table, and remove_small_objects, against the oracle; ``v`` a numpy array or a CUDA tensor."""
    host = v if isinstance(v, np.ndarray) else v.cpu().numpy()
    want, num = bo.label(host, connectivity)
    lab, n, tab = A.label(v, connectivity, return_num=True, return_table=True)
    as_np = (lambda t: t) if isinstance(v, np.ndarray) else (lambda t: t.cpu().numpy())
    got = as_np(lab)
    assert got.dtype == np.int32 and got.shape == want.shape and n == num and isinstance(n, int)
    assert np.array_equal(got, want)
    size, first, box = bo.table(want, num)
    for g, w in ((tab.size, size), (tab.first, first), (tab.box, box)):
        g = as_np(g)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    for m in sizes:
        kept = as_np(A.remove_small_objects(v, m, connectivity))
        assert kept.dtype == np.uint8 and np.array_equal(kept, bo.remove_small_objects(host, m, connectivity))


@pytest.mark.parametrize("name", NAMES)
def test_label_table_and_remove_small_objects(A, name):
    for connectivity in (1, 2, 3):
        check_label(A, volume(name), connectivity)


def test_label_of_a_tensor_stays_on_the_device(A):
    v = volume("noise30")
    t = torch.from_numpy(v.copy()).cuda().to(torch.float32) * 3.0          # any dtype: non-zero = foreground
    lab = A.label(t)
    assert lab.is_cuda and lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), bo.label(v, 3)[0])
    lab, num = A.label(t, 1, return_num=True)
    assert num.is_cuda and num.dtype == torch.int32 and num.dim() == 0 and int(num) == bo.label(v, 1)[1]
    assert A.label(t, 1, return_num="int")[1] == bo.label(v, 1)[1]
    check_label(A, t, 2, sizes=(2,))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("connectivity", [3, 1])
def test_euler_and_betti_numbers(A, name, connectivity):
    v = volume(name)
    chi = A.euler_number(v, connectivity)
    b = A.betti_numbers(v, connectivity)
    assert isinstance(chi, int) and all(isinstance(x, int) for x in b)
    assert chi == bo.euler_number(v, connectivity)
    assert b == bo.betti_numbers(v, connectivity)
    if name in bo.KNOWN:
        assert b == bo.KNOWN[name]


def check_error(A, pred, lab, patch, connectivity, want_tables):
    (tp, tiles), (tl, _) = want_tables
    got = A.betti_error(pred, lab, patch, connectivity, whole=True)
    from seunet_amd.components import mean_abs_error
    err = mean_abs_error(tp, tl)
    assert got.tiles == tiles
    assert got.pred.is_cuda and got.pred.dtype == torch.int32 and tuple(got.pred.shape) == tp.shape
    assert np.array_equal(got.pred.cpu().numpy(), tp) and np.array_equal(got.label.cpu().numpy(), tl)
    assert got.error.dtype == np.float64 and np.array_equal(got.error, err) and got.total_error == float(err.sum())
    assert got.whole == (bo.betti_numbers(pred, connectivity), bo.betti_numbers(lab, connectivity))


@pytest.mark.parametrize("patch", bo.TILE_PATCHES + [7])
@pytest.mark.parametrize("connectivity", [3, 1])
def test_betti_error_over_tiles_of_noise(A, patch, connectivity):
    p = (patch,) * 3 if isinstance(patch, int) else patch
    check_error(A, bo.tile_volume("sparse"), bo.tile_volume("dense"), patch, connectivity,
                (bo.tile_tables("sparse", p, connectivity), bo.tile_tables("dense", p, connectivity)))


@pytest.mark.parametrize("patch", bo.TILE_PATCHES)
@pytest.mark.parametrize("connectivity", [3, 1])
def test_betti_error_of_shapes_across_a_tile_corner(A, patch, connectivity):
    check_error(A, bo.tile_volume("shapes"), bo.tile_volume("sparse"), patch, connectivity,
                (bo.tile_tables("shapes", patch, connectivity), bo.tile_tables("sparse", patch, connectivity)))


def test_betti_error_of_the_whole_volume(A):
    pred, lab = volume("torus"), volume("shell_with_ball")
    got = A.betti_error(pred, lab)
    assert got.tiles == (1, 1, 1) and got.whole is None
    assert got.pred.cpu().numpy().tolist() == [[1, 1, 0]] and got.label.cpu().numpy().tolist() == [[2, 0, 1]]
    assert got.error.tolist() == [1.0, 1.0, 1.0] and got.total_error == 3.0
    same = A.betti_error(torch.from_numpy(pred.copy()).cuda(), torch.from_numpy(pred.copy()).cuda(), patch=8)
    assert same.total_error == 0.0 and same.tiles == (4, 4, 4)
