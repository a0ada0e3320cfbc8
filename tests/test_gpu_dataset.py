"""GPU checks of the device-side batch builder (-m gpu): ag_fps_batch, ag_dataset_assemble, ag_build_edges_graphs and
adaptigraph_amd.DeviceDynDataset against tests/dataset_restate.py and the fixtures recorded from the reference's
DynDataset.__getitem__ (tests/golden/dataset_*.npz), then TrainStep on the batches and the prefetching loader."""
import numpy as np
import pytest
import torch

import dataset_restate as DR
import train_restate as TR
from test_gpu_train import _model

pytestmark = pytest.mark.gpu

BIT_EXACT = ["dataset_cloth", "dataset_granular", "dataset_backoff"]
TENSORS = ["state", "action", "eef_future", "action_future", "state_future"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. ag_fps_batch
def _cloud(kind, n, rng):
    if kind == "dup":
        return np.repeat(rng.normal(size=(1, 3)), n, 0).astype(np.float32)
    if kind == "grid":                                       # many exactly equal distances: ties everywhere
        g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
        return (g[np.arange(n) % 1000] * 0.125).astype(np.float32)
    return (rng.normal(size=(n, 3)) * [1.0, 0.1, 0.6]).astype(np.float32)


def _fps_cases(sizes, rng, max_nobj):
    """(cloud, fps_start, radius, rad_start) per sample: every size with its starts at both ends, radius 0 (every stage-1 point),
    a radius above the cloud (one point) and a usual one."""
    out = []
    for n in sizes:
        n1 = min(n, max_nobj)
        c = _cloud("rand", n, rng)
        out += [(c, 0, 0.3, n1 - 1), (c, n - 1, 0.0, 0), (c, n // 2, 100.0, n1 // 2), (_cloud("grid", n, rng), n - 1, 0.26, 0),
                (_cloud("dup", n, rng), n // 3, 0.0, n1 - 1)]
    return out


def _run_fps(dev, cases, max_nobj, max_pts):
    from adaptigraph_amd.dataset import fps_batch
    off = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])])
    pos = torch.from_numpy(np.concatenate([c[0] for c in cases])).to(dev)
    tab = torch.from_numpy(np.stack([off[:-1], [len(c[0]) for c in cases]], 1).astype(np.int64)).to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)   # noqa: E731
    idx, n_obj = fps_batch(pos, tab[:, 0], tab[:, 1], i32([c[1] for c in cases]),
                           torch.tensor([c[2] for c in cases], dtype=torch.float32, device=dev), i32([c[3] for c in cases]),
                           max_nobj, max_pts)
    return idx.cpu().numpy(), n_obj.cpu().numpy()


def _check_fps(dev, cases, max_nobj, max_pts):
    idx, n_obj = _run_fps(dev, cases, max_nobj, max_pts)
    for b, (c, s, r, rs) in enumerate(cases):
        want = DR.fps_indices(c, max_nobj, s, r, rs)
        assert n_obj[b] == len(want), (b, len(c), s, r, rs, int(n_obj[b]), len(want))
        assert np.array_equal(idx[b, :len(want)], want), (b, len(c), s, r, rs)
        assert (idx[b, len(want):] == -1).all()


@pytest.mark.parametrize("sizes,max_nobj", [((1, 2, 37, 63, 64, 65, 600, 601), 100), ((65, 1025, 4096), 300), ((8192, 257), 100),
                                            ((1500,), 1024)])
def test_fps_batch_equals_the_restatement(dev, sizes, max_nobj):
    """One launch per kernel instantiation (clouds up to 1024, 4096 and 8192 points, the capacity limit), B = 40 / 15 / 10 / 5."""
    _check_fps(dev, _fps_cases(sizes, np.random.default_rng(len(sizes)), max_nobj), max_nobj, max(sizes))


def test_fps_batch_of_one_and_of_130(dev):
    rng = np.random.default_rng(5)
    _check_fps(dev, [(_cloud("rand", 600, rng), 17, 0.2, 3)], 100, 600)
    cases = [(_cloud("rand", int(n), rng), int(rng.integers(n)), float(rng.uniform(0.1, 0.4)), int(rng.integers(min(n, 100))))
             for n in rng.integers(1, 700, 130)]
    _check_fps(dev, cases, 100, 700)


def test_fps_above_the_limit_is_refused_before_anything_is_enqueued(dev):
    import adaptigraph_amd as ag
    from adaptigraph_amd import _lib
    from adaptigraph_amd.dataset import FPS_MAX_POINTS
    rng = np.random.default_rng(0)
    with pytest.raises(NotImplementedError, match=str(FPS_MAX_POINTS)):
        _run_fps(dev, [(_cloud("rand", FPS_MAX_POINTS + 1, rng), 0, 0.2, 0)], 100, FPS_MAX_POINTS + 1)
    eng = ag.default_engine(dev)                             # the C-ABI itself refuses too, with the limit in the message
    z = torch.zeros(8, dtype=torch.int64, device=dev)
    rc = eng.lib.ag_fps_batch(eng.ctx, None, z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), 1,
                              100, FPS_MAX_POINTS + 1, z.data_ptr(), z.data_ptr())
    assert rc == _lib.AG_ERR_UNSUPPORTED and str(FPS_MAX_POINTS) in eng.lib.ag_last_error(eng.ctx).decode()


# ------------------------------------------------------------------------------------------------ 2. batch() against the reference
_CACHE = {}


def _case(name, dev):
    """(fixture, dataset, draws, batch with dense Rr / Rs, trail) - built once per fixture."""
    import adaptigraph_amd as ag
    if name not in _CACHE:
        fx = DR.load_fixture(name)
        ds = ag.DeviceDynDataset(*DR.dataset_args(fx), device=dev)
        d = fx["draws"]
        t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)   # noqa: E731
        dr = ag.BatchDraws(t(d["fps_start"], torch.int32), t(d["fps_radius"], torch.float32), t(d["rad_start"], torch.int32),
                           t(d["phys_noise"], torch.float64), t(d["state_noise"], torch.float64), t(d["rot"], torch.float64),
                           t(d["adj_thresh"], torch.float64), t(d["knn_thresh"], torch.float64))
        data = ds.batch(fx["samples"], draws=dr, dense=True)
        _CACHE[name] = (fx, ds, dr, data, ds.last_trail)
    return _CACHE[name]


def _edges_of(el):
    n = el.n_edges.cpu().numpy()
    r, s, rp = el.recv.cpu().numpy(), el.send.cpu().numpy(), el.row_ptr.cpu().numpy()
    return n, [r[b, :n[b]] for b in range(len(n))], [s[b, :n[b]] for b in range(len(n))], rp


@pytest.mark.parametrize("name", ["dataset_rope", "dataset_cloth", "dataset_granular", "dataset_backoff", "dataset_softbody"])
def test_batch_equals_the_reference(dev, name):
    fx, ds, _, data, trail = _case(name, dev)
    want = fx["want"]
    B = len(fx["samples"])
    assert len(ds) == len(fx["pair_lists"]) and data["max_edges"] == ds.spec.max_nR
    pkey = fx["material"] + "_physics_param"
    for k in ("attrs", "p_rigid", "p_instance", "obj_mask", "material_index", pkey):
        got = data[k].cpu().numpy()
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), (name, k)
    for k in TENSORS:
        got = data[k].cpu().numpy()
        assert got.shape == want[k].shape and got.dtype == np.float32
        if name != "dataset_rope":
            assert np.array_equal(got.view(np.uint32), want[k].view(np.uint32)), (name, k)
        else:
            err = np.abs(got[..., :2].astype(np.float64) - want[k][..., :2])
            print(f"{name} {k}: max error {err.max():.3e}, smallest slack {(DR.rotation_bound(want[k]) - err).min():.3e}")
            assert np.array_equal(got[..., 2], want[k][..., 2]), (name, k)
            assert (err <= DR.rotation_bound(want[k])).all(), (name, k, float(err.max()))
    n, recv, send, row_ptr = _edges_of(data["edges"])
    assert np.array_equal(n, want["n_edges"]) and (n <= ds.spec.max_nR).all()
    N = data["attrs"].shape[1]
    for b in range(B):
        assert np.array_equal(recv[b], want["recv"][b]) and np.array_equal(send[b], want["send"][b]), (name, b)
        assert np.array_equal(row_ptr[b], np.concatenate([[0], np.cumsum(np.bincount(want["recv"][b], minlength=N))])), (name, b)
        assert [(float(a), int(k), int(c)) for a, k, c in trail[b]] == fx["trail"][b], (name, b, trail[b], fx["trail"][b])


@pytest.mark.parametrize("name", ["dataset_rope", "dataset_cloth", "dataset_granular", "dataset_backoff", "dataset_softbody"])
def test_dense_relations_equal_the_reference_row_for_row(dev, name):
    fx, ds, _, data, _ = _case(name, dev)
    want = fx["want"]
    B, N, E = len(fx["samples"]), data["attrs"].shape[1], ds.spec.max_nR
    Rr, Rs = np.zeros((B, E, N), np.float32), np.zeros((B, E, N), np.float32)
    for b in range(B):
        e = np.arange(len(want["recv"][b]))
        Rr[b, e, want["recv"][b]] = 1
        Rs[b, e, want["send"][b]] = 1
    assert np.array_equal(data["Rr"].cpu().numpy(), Rr) and np.array_equal(data["Rs"].cpu().numpy(), Rs)


def _lowered(name, dev, max_nR):
    """The fixture's dataset with max_nR lowered, and its constructor arguments."""
    import copy
    import adaptigraph_amd as ag
    fx, _, dr, _, _ = _case(name, dev)
    args = [copy.deepcopy(a) for a in DR.dataset_args(fx)]
    args[0]["datasets"][0]["max_nR"] = max_nR
    return fx, args, dr, ag.DeviceDynDataset(*args, device=dev)


def test_knn_back_off_of_the_per_sample_path(dev):
    """softbody with max_nR 700 instead of 3500: by the restatement (pinned to the reference on the CPU) one graph fits at once, one
    lowers its kNN fraction only, one lowers kNN to its minimum and then top-k three times.  Edges and trail equal."""
    fx, args, dr, ds = _lowered("dataset_softbody", dev, 700)
    want = DR.restate_batch(*args, fx["samples"], fx["draws"])
    assert sorted(len(t) for t in want["trail"]) == [1, 2, 4]
    assert any(t[-1][0] < t[0][0] and t[-1][1] == t[0][1] for t in want["trail"]) and any(t[-1][1] < t[0][1] for t in want["trail"])
    data = ds.batch(fx["samples"], draws=dr)
    n, recv, send, _ = _edges_of(data["edges"])
    assert (n <= 700).all() and data["max_edges"] == 700
    for b in range(len(n)):
        assert np.array_equal(recv[b], want["recv"][b]) and np.array_equal(send[b], want["send"][b]), b
        assert [(float(a), int(k), int(c)) for a, k, c in ds.last_trail[b]] == [tuple(r) for r in want["trail"][b]], b


def test_top_k_reaching_zero_raises_exceeds_max_dims(dev):
    """granular with max_nR 1: no top-k fits (a graph keeps at least its self-loops), so the back-off ends in the reference's
    Exception('Exceeds max dims') instead of looping."""
    fx, _, dr, ds = _lowered("dataset_granular", dev, 1)
    with pytest.raises(Exception, match="Exceeds max dims"):
        ds.batch(fx["samples"], draws=dr)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. into TrainStep and the model
def _reference_dict(fx, dev, max_nR):
    """The fixture's own collated batch with dense Rr / Rs, as the reference's DataLoader would hand it over."""
    want = fx["want"]
    B, N = want["attrs"].shape[:2]
    d = {k: torch.from_numpy(want[k]).to(dev) for k in TENSORS + ["attrs", "p_rigid", "p_instance", "obj_mask", "material_index"]}
    pkey = fx["material"] + "_physics_param"
    d[pkey] = torch.from_numpy(want[pkey]).to(dev)
    Rr, Rs = torch.zeros((B, max_nR, N), device=dev), torch.zeros((B, max_nR, N), device=dev)
    for b in range(B):
        e = torch.arange(len(want["recv"][b]), device=dev)
        Rr[b, e, torch.from_numpy(want["recv"][b]).to(dev).long()] = 1
        Rs[b, e, torch.from_numpy(want["send"][b]).to(dev).long()] = 1
    d["Rr"], d["Rs"] = Rr, Rs
    return d


@pytest.mark.parametrize("name", BIT_EXACT)
def test_train_step_on_the_batch_equals_train_step_on_the_reference_batch(dev, name):
    """Three TrainStep.step on ds.batch(...) and on the fixture's dict with dense Rr / Rs: the same loss bits, the same weights;
    and DynamicsPredictor(**data) takes the dict as it is."""
    import adaptigraph_amd as ag
    fx, ds, dr, _, _ = _case(name, dev)
    W = TR.make_weights(3, n_his=ds.spec.n_his)
    ours = ag.TrainStep(_model(dev, W, n_his=ds.spec.n_his, material=fx["material"]), n_future=ds.spec.n_future)
    theirs = ag.TrainStep(_model(dev, W, n_his=ds.spec.n_his, material=fx["material"]), n_future=ds.spec.n_future)
    ref = _reference_dict(fx, dev, ds.spec.max_nR)
    for it in range(3):
        data = ds.batch(fx["samples"], draws=dr)
        a = ours.step(data, max_edges=data["max_edges"])
        b = theirs.step(ref, max_edges=ds.spec.max_nR)
        print(f"{name} step {it}: loss {a.item():.9g} / {b.item():.9g}")
        assert a.view(torch.int32).item() == b.view(torch.int32).item()
    ours.check()
    theirs.check()
    for w0, w1 in zip(ours.w, theirs.w):
        assert torch.equal(w0, w1)
    e0, e1 = ours.evaluate(data, max_edges=data["max_edges"]), theirs.evaluate(ref, max_edges=ds.spec.max_nR)
    assert e0.view(torch.int32).item() == e1.view(torch.int32).item()
    model = _model(dev, W, n_his=ds.spec.n_his, material=fx["material"])
    p0, p1 = model(**data), model(**ref)
    assert torch.equal(p0[0], p1[0]) and torch.equal(p0[1], p1[1])


def test_step_on_a_batch_does_not_wait_for_the_gpu(dev):
    """TrainStep.step(ds.batch(...), max_edges=ds.max_nR) only enqueues: it returns while an earlier kernel still spins."""
    import adaptigraph_amd as ag
    fx, ds, dr, data, _ = _case("dataset_cloth", dev)
    ts = ag.TrainStep(_model(dev, TR.make_weights(3), material=fx["material"]), n_future=ds.spec.n_future)
    for _ in range(2):
        ts.step(data, max_edges=data["max_edges"])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(10_000_000)
    e1.record()
    torch.cuda.synchronize()
    ms_per_cycle = e0.elapsed_time(e1) / 10_000_000
    done = torch.cuda.Event()
    torch.cuda._sleep(int(200.0 / ms_per_cycle))
    done.record()
    ts.step(data, max_edges=data["max_edges"])
    still_busy = not done.query()
    torch.cuda.synchronize()
    assert still_busy, "TrainStep.step waited for the GPU"
    ts.check()


# ------------------------------------------------------------------------------------------------ 4. the loader
def test_prefetching_loader_yields_the_same_batches(dev):
    """Five iterations with and without prefetch from generators seeded alike: every tensor and every edge bit-equal.  The rope
    config draws noise and a rotation, and six pairs in batches of four give a short batch and a second epoch."""
    _, ds, _, _, _ = _case("dataset_rope", dev)
    runs = []
    for prefetch in (False, True):
        g = torch.Generator(device=dev)
        g.manual_seed(11)
        it = ds.loader(4, True, generator=g, prefetch=prefetch)
        got = []
        for _ in range(5):
            d = next(it)
            torch.cuda.current_stream(dev).synchronize()      # everything the hand-over promised is then complete
            got.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()})
        it.close()
        runs.append(got)
    sizes = [d["state"].shape[0] for d in runs[0]]
    assert sizes == [4, 2, 4, 2, 4]
    for a, b in zip(*runs):
        assert a.keys() == b.keys()
        for k in a:
            if torch.is_tensor(a[k]):
                assert torch.equal(a[k], b[k]), k
        na, ra, sa, pa = _edges_of(a["edges"])
        nb, rb, sb, pb = _edges_of(b["edges"])
        assert np.array_equal(na, nb) and np.array_equal(pa, pb)
        assert all(np.array_equal(x, y) for x, y in zip(ra + sa, rb + sb))
    assert not torch.equal(runs[0][0]["state"], runs[0][2]["state"])          # the generator moved on


def test_default_draws_are_in_range(dev):
    """ds.draws: starts inside their clouds (the 37-point episode included), radii and thresholds inside the config's ranges."""
    fx, ds, _, _, _ = _case("dataset_rope", dev)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    idx = np.tile(np.arange(len(ds)), 40)
    dr = ds.draws(idx, generator=g)
    n_e = np.array([fx["obj_pos"][e].shape[1] for e in fx["pair_lists"][idx, 0]])
    s, r = dr.fps_start.cpu().numpy(), dr.rad_start.cpu().numpy()
    assert (s >= 0).all() and (s < n_e).all() and (r >= 0).all() and (r < np.minimum(n_e, ds.spec.max_nobj)).all()
    assert s[n_e == 37].max() > 30 and s[n_e == 37].min() < 6
    lo, hi = ds.spec.fps_radius_range
    rad = dr.fps_radius.cpu().numpy()
    assert rad.dtype == np.float32 and (rad >= np.float32(lo)).all() and (rad <= np.float32(hi)).all()
    adj = dr.adj_thresh.cpu().numpy()
    assert (adj >= ds.spec.adj_radius_range[0]).all() and (adj <= ds.spec.adj_radius_range[1]).all()
    assert dr.state_noise.shape == (len(idx), ds.spec.n_his, ds.N, 3) and float(dr.state_noise.abs().max()) <= ds.spec.state_noise
    assert float(dr.rot.abs().max()) <= np.pi and (dr.knn_thresh == 1).all() and float(dr.phys_noise.abs().max()) == 0.0
