"""The online-hard-mining pool on the GPU (csrc/pool.hip: select / scatter / gather; ``seunet_amd.OnlineHardPool``) against
tests/pool_oracle.py, the recorded behaviour of the reference (tests/golden/online_pool_known.npz) and bit-exact payloads.

Everything here is exact: slots, keys, sequence numbers and the state are integers or copied floats, payloads are compared as
integers (NaN payloads and -0.0 count).  Scatter / gather and the Python class run under tests/guarded_alloc.py: three fills of
every ``torch.empty`` (the pool's own storage among them), red zones around every buffer, inputs passed through ``guard()``,
results identical across the fills."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as G  # noqa: E402
from pool_oracle import PoolOracle  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "online_pool_known.npz")
SENTINEL_KEY, SENTINEL_SEQ = -12345.0, -777
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def L():
    import seunet_amd  # noqa: F401
    from seunet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- select ------------------------------------------------------------------------------------------------------------------
def guard(t):
    """Inside a red-zoned buffer when a guarded_allocations context is active (every test here runs its body under one)."""
    return G.guard(t) if G._active is not None else t


class DevicePool:
    """keys / seq / state on the device, driven through seunet_pool_select alone."""

    def __init__(self, L, capacity, oracle=None):
        self.L, self.capacity = L, capacity
        keys = [SENTINEL_KEY if oracle is None or k is None else k for k in (oracle.keys if oracle else [None] * capacity)]
        seq = [SENTINEL_SEQ if oracle is None or q is None else q for q in (oracle.seq if oracle else [None] * capacity)]
        state = [oracle.count, oracle.next] if oracle else [0, 0]      # (an oracle: a pool filled without a thousand launches)
        self.keys = guard(torch.tensor(keys, dtype=torch.float32, device="cuda"))
        self.seq = guard(torch.tensor(seq, dtype=torch.int64, device="cuda"))
        self.state = guard(torch.tensor(state, dtype=torch.int64, device="cuda"))

    def add(self, keys):
        from seunet_amd import _lib
        new = guard(torch.tensor(keys, dtype=torch.float32, device="cuda"))
        slots = guard(torch.full((len(keys),), -99, dtype=torch.int32, device="cuda"))
        _lib.check(self.L.seunet_pool_select(new.data_ptr(), len(keys), _lib.ptr(self.keys) if self.capacity else None,
                                             _lib.ptr(self.seq) if self.capacity else None, self.state.data_ptr(), self.capacity,
                                             slots.data_ptr(), _lib.stream_ptr()), "pool_select")
        return slots.tolist()

    def assert_equals(self, oracle, what):
        assert self.state.tolist() == [oracle.count, oracle.next], (what, self.state.tolist(), oracle.count, oracle.next)
        want_k = np.array([SENTINEL_KEY if k is None else k for k in oracle.keys], np.float32)
        want_q = np.array([SENTINEL_SEQ if q is None else q for q in oracle.seq], np.int64)
        assert np.array_equal(self.keys.cpu().numpy().view(np.int32), want_k.view(np.int32)), what
        assert np.array_equal(self.seq.cpu().numpy(), want_q), what


def key_stream(kind, calls, B, seed):
    """``calls`` lists of B float32 keys: ``random`` distinct-ish normals, ``ties`` drawn from 6 values; both with NaN, +inf
    and -inf mixed in."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(calls):
        if kind == "ties":
            k = rng.choice(np.array([0.0, -0.0, 0.25, 0.5, 0.5000001, 1.0], np.float32), B)
        else:
            k = rng.standard_normal(B).astype(np.float32)
        special = rng.random(B)
        k = np.where(special < 0.04, np.float32(NAN), np.where(special < 0.07, np.float32(INF), np.where(special < 0.1, np.float32(-INF), k)))
        out.append([float(v) for v in k.astype(np.float32)])
    return out


@pytest.mark.parametrize("kind", ("random", "ties"))
@pytest.mark.parametrize("B", (1, 3, 4, 32))
@pytest.mark.parametrize("capacity", (1, 7, 64, 1000))
def test_select_follows_the_oracle(L, capacity, B, kind):
    G.three_fills(lambda: select_run(L, capacity, B, kind), family="online_pool select")


def select_run(L, capacity, B, kind):
    oracle = PoolOracle(capacity)
    calls = 14
    prefill = max(0, capacity - 3 * B)             # the stream below then fills the rest, crosses "exactly full" and evicts
    if prefill:
        first = key_stream(kind, 1, prefill, seed=capacity)[0]
        first = [0.5 if not np.isfinite(v) else v for v in first]
        assert oracle.add(first) == list(range(prefill))
    dev = DevicePool(L, capacity, oracle)
    dev.assert_equals(oracle, "start")
    seen = set()
    for it, keys in enumerate(key_stream(kind, calls, B, seed=1000 * capacity + B)):
        full = oracle.count == capacity
        want = oracle.add(keys)
        got = dev.add(keys)
        assert got == want, (it, keys, got, want)
        dev.assert_equals(oracle, f"call {it}")
        seen.update(("full" if full else "filling", "skip" if s < 0 else "keep") for s in want)
    assert oracle.count == capacity and ("full", "keep") in seen
    if kind == "random" and B > 1 and capacity > 1:
        assert ("full", "skip") in seen
    return dev.keys.clone(), dev.seq.clone(), dev.state.clone()


def test_select_in_call_chain_ties_and_specials(L):
    G.three_fills(lambda: chain_run(L), family="online_pool select")


def chain_run(L):
    oracle = PoolOracle(2)
    dev = DevicePool(L, 2)
    for keys, want in (([5.0, 6.0], [0, 1]), ([7.0, 8.0, 9.0], [-1, 1, 0]),          # 7 takes a, 8 takes b, 9 takes a back from 7
                       ([8.0], [1]),                                                   # equal to the minimum: accepted
                       ([np.nextafter(np.float32(8.0), np.float32(0.0)).item()], [-1]),   # strictly below it: dropped
                       ([NAN, INF, -INF], [-1, -1, -1]), ([9.0, 9.0, 9.0], [-1, 0, 1]), ([9.0], [0])):
        assert oracle.add(keys) == want
        assert dev.add(keys) == want, keys
        dev.assert_equals(oracle, str(keys))
    return dev.keys.clone(), dev.seq.clone(), dev.state.clone()


def test_select_with_capacity_zero(L):
    def op():
        dev = DevicePool(L, 0)
        assert dev.add([1.0, NAN, 3.0]) == [-1, -1, -1] and dev.state.tolist() == [0, 0]
        return dev.state.clone()

    G.three_fills(op, family="online_pool select")


def test_entry_points_reject_bad_arguments(L):
    from seunet_amd import _lib
    import ctypes as C
    z = torch.zeros(64, device="cuda")
    p = z.data_ptr()
    assert L.seunet_pool_select(p, 0, p, p, p, 4, p, None) != 0 and "batch" in _lib.last_error()
    assert L.seunet_pool_select(p, 1, p, p, p, 65536, p, None) != 0 and "capacity" in _lib.last_error()
    assert L.seunet_pool_select(p, 1, None, None, p, 4, p, None) != 0
    assert L.seunet_pool_scatter(p, 1, 4, 24, p, p, p, None, p, p, p, None, None) != 0 and "multiple of 16" in _lib.last_error()
    assert L.seunet_pool_scatter(p, 1, 4, 16, p + 4, p, p, None, p, p, p, None, None) != 0 and "aligned" in _lib.last_error()
    assert L.seunet_pool_scatter(p, 1, 4, 16, p, p, p, p, p, p, p, None, None) != 0
    slots = (C.c_int * 2)(0, 4)
    assert L.seunet_pool_gather(slots, 2, 4, 16, p, p, p, None, p, p, p, None, None) != 0 and "outside the pool" in _lib.last_error()
    assert L.seunet_pool_gather(slots, 33, 4, 16, p, p, p, None, p, p, p, None, None) != 0
    import seunet_amd as A
    with pytest.raises(ValueError, match="multiple of 16"):
        A.OnlineHardPool(3, cube=6)
    pool = A.OnlineHardPool(2, cube=(1, 4, 4))
    with pytest.raises(ValueError):
        pool.add(torch.zeros(2, device="cuda"), torch.zeros(2, 2, 1, 4, 4, device="cuda"), torch.zeros(2, 1, 1, 4, 4, device="cuda"),
                 torch.zeros(2, 1, 1, 4, 3, device="cuda"))
    with pytest.raises(ValueError):
        pool.add(torch.zeros(2, device="cuda"), torch.zeros(2, 2, 1, 4, 4, device="cuda"), torch.zeros(2, 1, 1, 4, 4, device="cuda"),
                 torch.zeros(2, 1, 1, 4, 4, device="cuda"), skel=torch.zeros(2, 1, 1, 4, 4, device="cuda"))


# ---- scatter and gather, under guarded memory --------------------------------------------------------------------------------
PATTERN32, PATTERN8 = 0x5A5AA5A5, 0xC3


def bit_patterns(g, shape):
    """f32 tensor of random bit patterns (NaN payloads, infinities, subnormals among them) with -0.0 and a NaN planted."""
    bits = torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32)
    flat = bits.reshape(-1)
    flat[0], flat[-1] = -2 ** 31, 0x7FC00123                 # -0.0, a quiet NaN with a payload
    flat[1] = 0x7F800001                                       # a signalling NaN
    return bits.view(torch.float32)


def as_int(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("with_skel", (False, True), ids=("noskel", "skel"))
@pytest.mark.parametrize("shape", ((1, 4, 4), (2, 8, 37), (32, 32, 32)), ids=("V16", "V592", "V32768"))
def test_scatter_and_gather_bitwise(L, shape, with_skel):
    import seunet_amd as A
    V = shape[0] * shape[1] * shape[2]
    K, B = 6, 3
    calls = ([0.5, 0.1, 0.7], [0.2, NAN, 0.9], [0.05, 0.6, 0.3], [0.8, 0.8, 0.01], [1.0, 1.1, 1.2])

    def op():
        g = torch.Generator().manual_seed(7)
        pool = A.OnlineHardPool(K, cube=shape, with_skel=with_skel)
        pool.data.view(torch.int32).fill_(PATTERN32)
        pool.weight.view(torch.int32).fill_(PATTERN32)
        pool.label.fill_(PATTERN8)
        if with_skel:
            pool.skel.fill_(PATTERN8)
        oracle = PoolOracle(K)
        record = []
        for keys in calls:
            data, weight = bit_patterns(g, (B, 2) + shape), bit_patterns(g, (B, 1) + shape)
            label = (torch.rand((B, 1) + shape, generator=g) < 0.3).float()
            skel = label * (torch.rand((B, 1) + shape, generator=g) < 0.5).float() if with_skel else None
            payloads = [(as_int(data[i]), label[i].to(torch.uint8), as_int(weight[i]), None if skel is None else skel[i].to(torch.uint8)) for i in range(B)]
            want = oracle.add(keys, payloads)
            dev = [None if v is None else G.guard(v.cuda()) for v in (torch.tensor(keys), data, label, weight, skel)]
            got = pool.add(dev[0], dev[1], dev[2], dev[3], skel=dev[4])
            assert got.tolist() == want, (keys, got.tolist(), want)
            pd, pl, pw = as_int(pool.data).reshape(K, 2, *shape), pool.label.cpu().reshape(K, 1, *shape), as_int(pool.weight).reshape(K, 1, *shape)
            ps = pool.skel.cpu().reshape(K, 1, *shape) if with_skel else None
            for j in range(K):
                if j < oracle.count:                     # every occupied slot holds the oracle's sample, bit for bit
                    d, lab, w, s = oracle.payload[j]
                    assert torch.equal(pd[j], d) and torch.equal(pl[j], lab) and torch.equal(pw[j], w), (keys, j)
                    assert ps is None or torch.equal(ps[j], s)
                else:                                    # a never-used slot keeps the pattern
                    assert bool((pd[j] == PATTERN32).all()) and bool((pw[j] == PATTERN32).all()) and bool((pl[j] == PATTERN8).all())
                    assert ps is None or bool((ps[j] == PATTERN8).all())
            record.append((got.clone(), pool.data.clone(), pool.label.clone(), pool.weight.clone(), None if ps is None else pool.skel.clone()))
        assert len(pool) == K
        rng = np.random.default_rng(3)
        for n in (1, 5, 32):
            slots = rng.integers(0, K, n).tolist()
            out = pool.gather(slots)
            assert out["data"].shape == (n, 2) + shape and out["label"].shape == (n, 1) + shape
            for i, j in enumerate(slots):
                d, lab, w, s = oracle.payload[j]
                assert torch.equal(as_int(out["data"][i]), d) and torch.equal(as_int(out["weight"][i]), w)
                assert torch.equal(out["label"][i].cpu(), lab.float())
                assert (s is None) == ("skel" not in out) and (s is None or torch.equal(out["skel"][i].cpu(), s.float()))
            record.append(out)
        return record

    G.three_fills(op, family=f"online_pool V={V}")


# ---- the recorded reference runs, through the Python class ------------------------------------------------------------------------
@pytest.mark.parametrize("run", range(12))
def test_fixture_runs_through_the_pool(L, run):
    import seunet_amd as A
    known = np.load(GOLDEN)
    three, B, K = (int(v) for v in known[f"run{run}_config"])
    keys, survivors = known[f"run{run}_keys"], known[f"run{run}_survivors"]
    shape = (1, 4, 4)

    def op():
        pool = A.OnlineHardPool(K, cube=shape, with_skel=bool(three))
        pool.clear()
        oracle = PoolOracle(K)
        alive = []
        for it in range(keys.shape[0]):
            ids = torch.arange(it * B, (it + 1) * B, dtype=torch.float32)
            data = torch.zeros((B, 2) + shape)
            data[:, 0, 0, 0, 0] = ids
            weight = data[:, :1] + 0.5
            label = (torch.arange(B * 16).reshape((B, 1) + shape) % 3 == 0).float()
            dev = [G.guard(v.cuda()) for v in (torch.from_numpy(keys[it]), data, label, weight)]
            slots = pool.add(*dev, skel=G.guard(label.cuda()) if three else None)
            assert slots.tolist() == oracle.add(keys[it].tolist(), list(range(it * B, (it + 1) * B)))
            n = len(pool)
            got = sorted(int(v) for v in pool.data[:n, 0, 0].tolist())
            assert got == [int(v) for v in survivors[it] if v >= 0], (it, got)
            alive.append(got)
        out = {"alive": alive}
        for k, rate in enumerate(known["rates"].tolist()):
            want = known[f"run{run}_replay{k}"].tolist()
            for bs in (1, 2):
                seed = 100 + k
                batches = list(pool.replay(batch_size=bs, rate=rate, generator=torch.Generator().manual_seed(seed)))
                ids = [[int(v) for v in b["data"][:, 0, 0, 0, 0].tolist()] for b in batches]
                flat = [v for b in ids for v in b]
                assert len(batches) == len(want) // bs and len(set(flat)) == len(flat) and set(flat) <= set(want)
                if bs == 1:
                    assert sorted(flat) == sorted(want), (rate, flat, want)                 # the reference's selection
                perm = torch.randperm(len(want), generator=torch.Generator().manual_seed(seed)).tolist()
                assert ids == [[oracle.payload[j] for j in b] for b in oracle.replay_batches(perm, bs, rate)]
                for b in batches:
                    assert torch.equal(b["weight"][:, 0, 0, 0, 0], b["data"][:, 0, 0, 0, 0] + 0.5) and (("skel" in b) == bool(three))
                out[f"replay{k}_{bs}"] = ids
        pool.clear()
        assert len(pool) == 0 and list(pool.replay()) == []
        return out

    G.three_fills(op, family="online_pool fixture")


def test_limit_zero_stores_nothing(L):
    import seunet_amd as A

    def op():
        pool = A.OnlineHardPool(0, cube=(1, 4, 4))
        z = torch.zeros(3, 1, 1, 4, 4, device="cuda")
        slots = pool.add(G.guard(torch.tensor([1.0, 2.0, 3.0], device="cuda")), G.guard(torch.zeros(3, 2, 1, 4, 4, device="cuda")), G.guard(z), G.guard(z))
        assert slots.tolist() == [-1, -1, -1] and len(pool) == 0 and list(pool.replay()) == []
        return slots.clone()

    G.three_fills(op, family="online_pool limit 0")


# ---- no synchronise ---------------------------------------------------------------------------------------------------------------
def test_key_and_add_do_not_synchronise(L):
    """torch.cuda.set_sync_debug_mode("error") makes every synchronising torch call raise; the mode is checked to bite first."""
    import seunet_amd as A
    shape = (16, 16, 16)
    pool = A.OnlineHardPool(3, cube=shape)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((4, 1) + shape, device="cuda", generator=g)
    t = (torch.rand((4, 1) + shape, device="cuda", generator=g) < 0.1).float()
    w = 1 + torch.rand((4, 1) + shape, device="cuda", generator=g)
    data = torch.randn((4, 2) + shape, device="cuda", generator=g)
    A.per_sample_loss(x, t, w, apply_sigmoid=True)                     # (the library is loaded before the mode is set)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            x.sum().item()
        for _ in range(2):
            keys = A.per_sample_loss(x, t, w, apply_sigmoid=True)
            pool.add(keys, data, t, w)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert len(pool) == 3 and bool(torch.isfinite(keys).all())


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", (2, 3))
def test_training_steps_feed_the_pool(L, stage):
    import seunet_amd as A
    import seunet_oracle as orc
    torch.manual_seed(0)
    m = A.SE_UNet(2, 1)
    m.load_state_dict(orc.deterministic_state_dict(2, 1, 1, 0))
    m = m.cuda()
    opt = A.AdamW(m.parameters(), lr=1e-4)
    pool = A.OnlineHardPool(limit=4, cube=32, with_skel=stage == 3)
    pool.clear()
    g = torch.Generator().manual_seed(stage)
    all_keys, crops, losses = [], [], []
    for step in range(3):
        data = torch.rand(2, 2, 32, 32, 32, generator=g).cuda()
        label = (data[:, 0:1] > 0.9).float()
        weight = 1 + torch.rand(2, 1, 32, 32, 32, generator=g).cuda()
        skel = label * (data[:, 1:2] > 0.5).float() if stage == 3 else None
        opt.zero_grad(set_to_none=True)
        pred_en, pred_de = m(data)
        loss = A.fused_stage_loss(stage, pred_en, pred_de, label, weight, skel)
        loss.backward()
        opt.step()
        keys = A.per_sample_loss(pred_de, label, weight, apply_sigmoid=True)
        pool.add(keys, data, label, weight, skel=skel)
        losses.append(float(loss.detach()))
        all_keys += keys.tolist()
        crops += [(data[i], label[i], weight[i], None if skel is None else skel[i]) for i in range(2)]
    assert len(pool) == 4 and all(np.isfinite(v) for v in losses + all_keys), (losses, all_keys)
    stored, seq = pool.snapshot()
    assert sorted(stored.tolist()) == sorted(all_keys)[-4:], (stored.tolist(), all_keys)       # the four largest of the six keys
    # one replay step with batch 1: the replayed tensors are bitwise the stored crops
    batch = next(iter(pool.replay(batch_size=1, generator=torch.Generator().manual_seed(9))))
    src = [c for c in crops if torch.equal(c[0], batch["data"][0])]
    assert len(src) == 1 and torch.equal(src[0][1], batch["label"][0]) and torch.equal(src[0][2].view(torch.int32), batch["weight"][0].view(torch.int32))
    assert (stage == 3) == ("skel" in batch) and (stage == 2 or torch.equal(src[0][3], batch["skel"][0]))
    opt.zero_grad(set_to_none=True)
    pred_en, pred_de = m(batch["data"])
    loss = A.fused_stage_loss(stage, pred_en, pred_de, batch["label"], batch["weight"], batch.get("skel"))
    loss.backward()
    opt.step()
    assert np.isfinite(float(loss.detach()))
