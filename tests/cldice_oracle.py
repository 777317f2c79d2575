"""The definition of the soft skeleton, the soft clDice loss (Shit et al., "clDice -- a Novel Topology-Preserving Loss Function
for Tubular Structure Segmentation", CVPR 2021) and the hard clDice score, torch / numpy on the CPU.

    erode(x)  = min over the 7-point cross (centre, +-1 along each of the 3 axes); outside the volume counts as +inf
    dilate(x) = max over the 3x3x3 box; outside the volume counts as -inf
    E_0 = x, E_{j+1} = erode(E_j);  O_j = dilate(E_{j+1});  d_j = relu(E_j - O_j)        j = 0..iters
    S_0 = d_0;  S_j = S_{j-1} + relu(d_j - S_{j-1}*d_j)                                  j = 1..iters
    soft_skeleton(x, iters) = S_iters
    tprec = (sum S(p) t + smooth) / (sum S(p) + smooth);  tsens = (sum S(t) p + smooth) / (sum S(t) + smooth)
    soft_cldice_loss = 1 - 2 tprec tsens / (tprec + tsens)          sums over the WHOLE batch

Tensors are (volumes, D, H, W): every leading index is a volume of its own.  relu'(0) = 0: all masks are strict ``> 0``.

Two statements of it:

(a) ``soft_skeleton_a`` / ``loss_and_grad_a``: the usual ``max_pool3d`` composition under torch autograd, in the dtype of the
    input (float64 or float32).  Where two voxels of a window hold the same value autograd's choice is torch's business (the
    elementwise ``torch.min`` even halves the gradient), so (a) defines the gradient on inputs with DISTINCT values only.  There
    min and max merely select, every route from a tie between routes ends at the same source voxel, and the gradient does not
    depend on any tie rule.

(b) ``forward_b`` / ``loss_and_grad_b``: an explicit forward that records its choices and the explicit backward through them.
    ``erode`` takes the FIRST minimum in the order (d-1, d, d+1, h-1, h+1, w-1, w+1), ``dilate`` the FIRST maximum in raster
    order of the box.  On tied inputs (binary masks, saturated or rounded probabilities) (b) alone is the definition.

    G = dL/dS_iters (from tprec);  gS = G
    for j = iters..1: m = [d_j - S_{j-1} d_j > 0];  gd_j = gS m (1 - S_{j-1});  gS = gS - gS m d_j
    gd_0 = gS;  gE = 0
    for j = iters..0: a = gd_j [E_j - O_j > 0];  gE' = gE + dilate^T(-a; argmax of O_j);  gE = a + erode^T(gE'; argmin of E_{j+1})
    dL/dp = gE + (dL/dtsens) S(t) / (sum S(t) + smooth)

The forward is exact in float32: selections and single adds, subtracts and multiplies, so an implementation that does not
contract them into fused multiply-adds gives the float32 statement's bits.

Hard score (``cldice_score``): tprec = |S_P and V_L| / |S_P|, tsens = |S_L and V_P| / |S_L|, 2 tprec tsens / (tprec + tsens) in
float64, from the four integer counts.  EMPTY SKELETONS GIVE 0, not nan: a ratio whose skeleton is empty counts as 0 (a
prediction without a centreline has shown no topological precision, a label without one cannot be covered), and so does the
score when both ratios are 0.  A metric that is averaged over the cases of a table must not turn the whole column into nan
because one case came out empty, and 0 is the value the score approaches as the overlap vanishes.
"""
import numpy as np
import torch
import torch.nn.functional as F

CROSS = ((-1, 0, 0), (0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
BOX = tuple((dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
MAX_ITERS = 16


# ---- (a) the max_pool3d composition ---------------------------------------------------------------------------------------------
def erode_a(x):
    p1 = -F.max_pool3d(-x, (3, 1, 1), (1, 1, 1), (1, 0, 0))
    p2 = -F.max_pool3d(-x, (1, 3, 1), (1, 1, 1), (0, 1, 0))
    p3 = -F.max_pool3d(-x, (1, 1, 3), (1, 1, 1), (0, 0, 1))
    return torch.min(torch.min(p1, p2), p3)


def dilate_a(x):
    return F.max_pool3d(x, 3, 1, 1)


def soft_skeleton_a(x, iters):
    e, s = x, None
    for j in range(iters + 1):
        e1 = erode_a(e)
        d = F.relu(e - dilate_a(e1))
        s = d if j == 0 else s + F.relu(d - s * d)
        e = e1
    return s


def value_from_sums(s0, s1, s2, s3, smooth):
    tprec = (s0 + smooth) / (s1 + smooth)
    tsens = (s2 + smooth) / (s3 + smooth)
    return 1 - 2 * tprec * tsens / (tprec + tsens)


def loss_and_grad_a(p, t, iters=3, smooth=1.0, dtype=torch.float64):
    """(loss, dL/dp, the four sums) of statement (a) in ``dtype``."""
    p = p.detach().to(dtype).clone().requires_grad_(True)
    t = t.detach().to(dtype)
    sp = soft_skeleton_a(p, iters)
    with torch.no_grad():
        st = soft_skeleton_a(t, iters)
    sums = ((sp * t).sum(), sp.sum(), (st * p).sum(), st.sum())
    loss = value_from_sums(*sums, smooth)
    loss.backward()
    return loss.detach(), p.grad.detach(), torch.stack([s.detach() for s in sums])


# ---- (b) explicit choices -----------------------------------------------------------------------------------------------------
def _shifted(x, offsets, fill):
    xp = F.pad(x, (1, 1, 1, 1, 1, 1), value=fill)
    D, H, W = x.shape[-3:]
    for dz, dy, dx in offsets:
        yield xp[..., 1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def _first(x, offsets, fill, smaller):
    """(value, index into ``offsets``) of the first extremum among the shifted copies of x."""
    best, idx = None, None
    for k, v in enumerate(_shifted(x, offsets, fill)):
        if best is None:
            best, idx = v.clone(), torch.zeros(x.shape, dtype=torch.int64)
            continue
        take = (v < best) if smaller else (v > best)
        best = torch.where(take, v, best)
        idx = torch.where(take, torch.full_like(idx, k), idx)
    return best, idx


def erode_b(x):
    return _first(x, CROSS, float("inf"), True)


def dilate_b(x):
    return _first(x, BOX, float("-inf"), False)


def _transpose(g, idx, offsets):
    """out[v + offsets[idx[v]]] += g[v]: the transpose of a selection."""
    D, H, W = g.shape[-3:]
    acc = torch.zeros(g.shape[:-3] + (D + 2, H + 2, W + 2), dtype=g.dtype)
    for k, (dz, dy, dx) in enumerate(offsets):
        acc[..., 1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] += torch.where(idx == k, g, torch.zeros_like(g))
    return acc[..., 1:1 + D, 1:1 + H, 1:1 + W]


def forward_b(x, iters):
    """(S_iters, state): state holds d_j, S_j and the recorded choices of every iteration."""
    e, s, st = x, None, {"d": [], "s": [], "amin": [], "amax": []}
    for j in range(iters + 1):
        e1, amin = erode_b(e)
        o, amax = dilate_b(e1)
        diff = e - o
        d = torch.where(diff > 0, diff, torch.zeros_like(diff))
        if j == 0:
            s = d
        else:
            r = d - s * d
            s = s + torch.where(r > 0, r, torch.zeros_like(r))
        st["d"].append(d); st["s"].append(s); st["amin"].append(amin); st["amax"].append(amax)
        e = e1
    return s, st


def soft_skeleton_b(x, iters):
    return forward_b(x, iters)[0]


def backward_b(G, st, iters):
    """dL/dx from G = dL/dS_iters."""
    gs = G
    gd = [None] * (iters + 1)
    for j in range(iters, 0, -1):
        d, sp = st["d"][j], st["s"][j - 1]
        m = (d - sp * d > 0).to(G.dtype)
        gd[j] = gs * m * (1 - sp)
        gs = gs - gs * m * d
    gd[0] = gs
    ge = torch.zeros_like(G)
    for j in range(iters, -1, -1):
        a = gd[j] * (st["d"][j] > 0).to(G.dtype)
        gep = ge + _transpose(-a, st["amax"][j], BOX)
        ge = a + _transpose(gep, st["amin"][j], CROSS)
    return ge


def loss_and_grad_b(p, t, iters=3, smooth=1.0, dtype=torch.float64, target_skeleton=None):
    """(loss, dL/dp, the four sums) of statement (b) in ``dtype``."""
    p, t = p.detach().to(dtype), t.detach().to(dtype)
    sp, state = forward_b(p, iters)
    st = soft_skeleton_b(t, iters) if target_skeleton is None else target_skeleton.to(dtype)
    s0, s1, s2, s3 = (sp * t).sum(), sp.sum(), (st * p).sum(), st.sum()
    a, b, c, d = s0 + smooth, s1 + smooth, s2 + smooth, s3 + smooth
    tprec, tsens = a / b, c / d
    den = tprec + tsens
    loss = 1 - 2 * tprec * tsens / den
    dl_dtprec, dl_dtsens = -2 * tsens * tsens / (den * den), -2 * tprec * tprec / (den * den)
    G = dl_dtprec * (t * b - a) / (b * b)
    grad = backward_b(G, state, iters) + dl_dtsens * st / d
    return loss, grad, torch.stack([s0, s1, s2, s3])


# ---- the hard score ---------------------------------------------------------------------------------------------------------
def cldice_counts(pred_mask, label_mask, pred_skeleton, label_skeleton):
    vp, vl, sp, sl = (np.asarray(v) != 0 for v in (pred_mask, label_mask, pred_skeleton, label_skeleton))
    return int((sp & vl).sum()), int(sp.sum()), int((sl & vp).sum()), int(sl.sum())


def score_from_counts(c0, c1, c2, c3):
    tprec = np.float64(c0) / np.float64(c1) if c1 else np.float64(0.0)
    tsens = np.float64(c2) / np.float64(c3) if c3 else np.float64(0.0)
    if tprec + tsens == 0:
        return 0.0, float(tprec), float(tsens)
    return float(2.0 * tprec * tsens / (tprec + tsens)), float(tprec), float(tsens)


def cldice_score(pred_mask, label_mask, pred_skeleton, label_skeleton):
    """(score, tprec, tsens) from masks and their skeletons (module docstring; empty skeletons give 0)."""
    return score_from_counts(*cldice_counts(pred_mask, label_mask, pred_skeleton, label_skeleton))


def tube_case():
    """(label, its centreline, a prediction with a side leak, that prediction's centreline): uint8 (9, 9, 20), hand-made"""
    label = np.zeros((9, 9, 20), np.uint8)
    label[3:6, 3:6, 2:18] = 1                            # a straight tube of radius 1 ...
    skel = np.zeros_like(label)
    skel[4, 4, 3:17] = 1                                 # ... and its centreline
    leak, leak_skel = label.copy(), skel.copy()
    leak[4, 6:9, 10] = 1                                 # a side leak: a twig that leaves the label ...
    leak_skel[4, 5:9, 10] = 1                            # ... and whose centreline leaves it with it
    return label, skel, leak, leak_skel


# ---- the test inputs ------------------------------------------------------------------------------------------------------
PARITY_SHAPES = ((2, 7, 9, 11), (3, 5, 33, 70), (1, 40, 24, 72))
DEGENERATE_SHAPES = ((1, 1, 1, 1), (1, 2, 3, 5))
ITERS = (0, 1, 3, 6)


def tubes(shape, seed, walks=3):
    """float32 (volumes, D, H, W) 0/1 target: a few random-walk tubes of radius 1 per volume."""
    rng = np.random.RandomState(seed)
    V, D, H, W = shape
    t = np.zeros(shape, dtype=np.float32)
    dims = np.array([D, H, W])
    for v in range(V):
        for _ in range(walks):
            pos = np.array([rng.randint(0, n) for n in dims])
            axis = int(np.argmax(dims))
            for _ in range(int(dims.max()) * 2):
                lo, hi = np.maximum(pos - 1, 0), np.minimum(pos + 2, dims)
                t[v, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1.0
                if rng.rand() < 0.3:
                    axis = rng.randint(0, 3)
                pos[axis] += rng.choice((-1, 1)) if rng.rand() < 0.2 else 1
                pos = np.clip(pos, 0, dims - 1)
    return torch.from_numpy(t)


def prediction(t, seed):
    """float32 prediction with DISTINCT values correlated with the target: the ranks of 0.7 blur(t) + 0.3 uniform, as
    (rank + 0.5) / n."""
    g = torch.Generator().manual_seed(seed)
    blur = sum(_shifted(t.double(), BOX, 0.0)) / 27          # the 3x3x3 box mean, zeros outside (any extent, also 1)
    field = 0.7 * blur + 0.3 * torch.rand(t.shape, generator=g, dtype=torch.float64)
    n = field.numel()
    assert n < 2 ** 23
    rank = torch.empty(n, dtype=torch.int64)
    rank[torch.argsort(field.reshape(-1), stable=True)] = torch.arange(n)
    p = ((rank.double() + 0.5) / n).float().reshape(t.shape)
    assert torch.unique(p).numel() == n
    return p


def sparse_target(shape):
    t = torch.zeros(shape, dtype=torch.float32)
    t.reshape(-1)[::3] = 1.0
    return t


_CASES = {}


def case(shape, seed=0):
    """(p, t) float32 for a shape, made once."""
    key = (tuple(shape), seed)
    if key not in _CASES:
        t = sparse_target(shape) if tuple(shape) in DEGENERATE_SHAPES else tubes(shape, 100 + seed)
        _CASES[key] = (prediction(t, 200 + seed), t)
    return _CASES[key]


_REF = {}


def reference(shape, iters, seed=0):
    """dict of the oracle runs on case(shape): float64 (a), float32 (a), made once and shared by the tests.  For the three
    parity shapes it asserts, on the float64 run alone, that the case is worth testing: 0.05 < loss < 1 - 1e-4 and a non-zero
    gradient on at least 40 % of the voxels."""
    key = (tuple(shape), iters, seed)
    if key not in _REF:
        p, t = case(shape, seed)
        l64, g64, s64 = loss_and_grad_a(p, t, iters, 1.0, torch.float64)
        l32, g32, s32 = loss_and_grad_a(p, t, iters, 1.0, torch.float32)
        if tuple(shape) in PARITY_SHAPES:
            share = float((g64 != 0).double().mean())
            assert 0.05 < float(l64) < 1 - 1e-4, (shape, iters, float(l64))
            assert share >= 0.4, (shape, iters, share)
        _REF[key] = {"l64": l64, "g64": g64, "s64": s64, "l32": l32, "g32": g32, "s32": s32}
    return _REF[key]


def tied_inputs(shape, seed=0):
    """the two tied predictions of a case: binary, and rounded to one decimal"""
    p, t = case(shape, seed)
    return (p > 0.6).float(), torch.round(p * 10) / 10, t


def rel_max(g, ref):
    return float((g.double() - ref.double()).abs().max() / ref.double().abs().max())
