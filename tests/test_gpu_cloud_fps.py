"""GPU checks (-m gpu) of ag_fps_cloud and adaptigraph_amd.perception: the sampler for clouds beyond LDS against
tests/dataset_restate.py (whose stage 1 is dgl's CPU sampler as remembered - see there) and against ag_fps_batch where both apply,
construct_graph / state_cur_from_points against tests/cloud_restate.py.  Every check is an equality of integer indices or of the
bits of gathered fp32 values."""
import numpy as np
import pytest
import torch

import cloud_restate as CR
import dataset_restate as DR
from adaptigraph_amd.perception import CLOUD_MAX_POINTS, CLOUD_SWITCH_POINTS as S, CLOUD_WG as W
from test_gpu_dataset import _cloud, _fps_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(dev, cases, max_nobj, max_pts, fn=None):
    """cases: (cloud, fps_start, radius, rad_start) per cloud of one launch of `fn` (fps_cloud unless given)."""
    from adaptigraph_amd.perception import fps_cloud
    sizes = [len(c[0]) for c in cases]
    off = np.concatenate([[0], np.cumsum(sizes)])
    pos = torch.from_numpy(np.concatenate([c[0] for c in cases])).to(dev)
    tab = torch.from_numpy(np.stack([off[:-1], sizes], 1).astype(np.int64)).to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)   # noqa: E731
    idx, n_obj = (fn or fps_cloud)(pos, tab[:, 0], tab[:, 1], i32([c[1] for c in cases]),
                                   torch.tensor([c[2] for c in cases], dtype=torch.float32, device=dev), i32([c[3] for c in cases]),
                                   max_nobj, max_pts)
    return idx.cpu().numpy(), n_obj.cpu().numpy()


def _check(dev, cases, max_nobj, max_pts):
    idx, n_obj = _run(dev, cases, max_nobj, max_pts)
    for b, (c, s, r, rs) in enumerate(cases):
        want = DR.fps_indices(c, max_nobj, s, r, rs) if len(c) else np.zeros(0, np.int64)
        assert n_obj[b] == len(want), (b, len(c), s, r, rs, int(n_obj[b]), len(want))
        assert np.array_equal(idx[b, :len(want)], want), (b, len(c), s, r, rs)
        assert (idx[b, len(want):] == -1).all()


# ------------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("sizes,max_nobj", [((1, 2, W - 1, W, W + 1), 100), ((8192, 8193, S - 1, S, S + 1), 100), ((100_000,), 100),
                                            ((CLOUD_MAX_POINTS,), 16), ((1500,), 1024)])
def test_fps_cloud_equals_the_restatement(dev, sizes, max_nobj):
    """Per size: both starts at the ends, radius 0, a radius above the cloud, a usual one, a grid and a cloud of one repeated point
    (ties).  Sizes around the workgroup (W), around ag_fps_batch's limit, around the register / workspace switch (S), a usual
    perceived cloud, the limit, and the largest max_nobj."""
    _check(dev, _fps_cases(sizes, np.random.default_rng(len(sizes) + max_nobj), max_nobj), max_nobj, max(sizes))


def test_one_launch_of_clouds_of_every_kind(dev):
    """An empty cloud, clouds with their minima in registers and clouds that use the workspace in one grid, and max_pts above all."""
    rng = np.random.default_rng(7)
    cases = [(_cloud("rand", n, rng), s, r, rs) for n, s, r, rs in
             [(0, 0, 0.2, 0), (1, 0, 0.2, 0), (300, 299, 0.25, 99), (8193, 17, 0.3, 5), (70_000, 69_999, 0.2, 0)]]
    cases.append((_cloud("grid", S + 4 * W + 3, rng), S + 1, 0.26, 50))               # ties across the switch
    _check(dev, cases, 100, 80_000)


def test_starts_out_of_range_are_clamped_and_a_count_above_max_pts_is_truncated(dev):
    rng = np.random.default_rng(8)
    c = _cloud("rand", 5000, rng)
    idx, n_obj = _run(dev, [(c, -3, 0.3, 4000), (c, 10**6, 0.3, -1)], 100, 5000)
    for b, (s, rs) in enumerate([(0, 99), (4999, 0)]):
        want = DR.fps_indices(c, 100, s, 0.3, rs)
        assert n_obj[b] == len(want) and np.array_equal(idx[b, :len(want)], want)
    idx, n_obj = _run(dev, [(c, 4999, 0.3, 0)], 100, 3000)                            # max_pts is the caller's bound on the count
    want = DR.fps_indices(c[:3000], 100, 2999, 0.3, 0)
    assert n_obj[0] == len(want) and np.array_equal(idx[0, :len(want)], want)


# ------------------------------------------------------------------------------------------------ 2. against ag_fps_batch
@pytest.mark.parametrize("sizes,max_nobj", [((1, 2, 63, 64, 65, 600, 1024), 100), ((1025, 4096), 300), ((4097, 8192), 100),
                                            ((1500,), 1024)])
def test_fps_cloud_equals_fps_batch_where_both_apply(dev, sizes, max_nobj):
    """Every ag_fps_batch instantiation (clouds up to 1024, 4096 and 8192 points): equal outputs, padding included."""
    from adaptigraph_amd.dataset import fps_batch
    cases = _fps_cases(sizes, np.random.default_rng(len(sizes)), max_nobj)
    idx_c, n_c = _run(dev, cases, max_nobj, max(sizes))
    idx_b, n_b = _run(dev, cases, max_nobj, max(sizes), fn=fps_batch)
    assert np.array_equal(n_c, n_b) and np.array_equal(idx_c, idx_b)


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_above_the_limits_is_refused_before_anything_is_enqueued(dev):
    import adaptigraph_amd as ag
    from adaptigraph_amd import _lib
    z = torch.zeros(8, dtype=torch.int64, device=dev)
    i32 = z[:1].int()
    with pytest.raises(NotImplementedError, match=str(CLOUD_MAX_POINTS)):
        ag.fps_cloud(torch.zeros(4, 3, device=dev), z[:1], z[:1], i32, z[:1].float(), i32, 100, CLOUD_MAX_POINTS + 1)
    with pytest.raises(NotImplementedError, match="1024"):
        ag.fps_cloud(torch.zeros(4, 3, device=dev), z[:1], z[:1], i32, z[:1].float(), i32, 1025, 4)
    eng = ag.default_engine(dev)                             # the C-ABI itself refuses too, with the limit in the message
    before = eng.alloc_counts()
    for max_nobj, max_pts, limit in ((100, CLOUD_MAX_POINTS + 1, CLOUD_MAX_POINTS), (1025, 4, 1024)):
        rc = eng.lib.ag_fps_cloud(eng.ctx, None, z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                  1, max_nobj, max_pts, z.data_ptr(), z.data_ptr())
        assert rc == _lib.AG_ERR_UNSUPPORTED and str(limit) in eng.lib.ag_last_error(eng.ctx).decode()
    assert eng.alloc_counts() == before


# ------------------------------------------------------------------------------------------------ 4. construct_graph
def _objects(sizes, rng):
    return [((rng.normal(size=(n, 3)) * [1.0, 0.1, 0.6]) + [4.0 * j, 0, 0]).astype(np.float32) for j, n in enumerate(sizes)]


def _same_graph(got, want):
    for k in ("state", "obj_state", "obj_state_raw", "eef_state"):
        g = got[k].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == want[k].shape, (k, g.shape, want[k].shape)
        assert np.array_equal(g.view(np.uint32), want[k].view(np.uint32)), k
    for k in ("state_mask", "eef_mask"):
        assert got[k].dtype == torch.bool and np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert len(got["fps_idx_list"]) == len(want["fps_idx_list"])
    for g, w in zip(got["fps_idx_list"], want["fps_idx_list"]):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("sizes,radius,n_eef,where", [((20_000,), 0.6, 0, "host"), ((9000, 300), 0.8, 3, "host"),
                                                      ((9000, 300), 0.8, 0, "device")])
def test_construct_graph_equals_the_restatement(dev, sizes, radius, n_eef, where):
    """One object, and two whose sampled points together stay below max_nobj; numpy arrays and device tensors; all objects in ONE
    launch (the family's launch counter)."""
    import adaptigraph_amd as ag
    rng = np.random.default_rng(len(sizes))
    clouds = _objects(sizes, rng)
    eef = rng.normal(size=(n_eef, 3)).astype(np.float32) if n_eef else None
    draws = [(int(rng.integers(n)), int(rng.integers(100))) for n in sizes]
    want = CR.construct_graph(clouds if len(clouds) > 1 else clouds[0], radius, draws, eef_kps=eef)
    assert 1 < len(want["obj_state"]) < 100 and all(len(i) > 1 for i in want["fps_idx_list"])
    given = [torch.from_numpy(c).to(dev) for c in clouds] if where == "device" else clouds
    eng = ag.default_engine(dev)
    eng.set_profiling(["fps"])
    try:
        eng.reset_stats()
        got = ag.construct_graph(given if len(given) > 1 else given[0], radius, eef_kps=eef, device=dev, draws=draws)
        assert eng.kernel_stats("fps")[1] == 1
    finally:
        eng.set_profiling([])
    _same_graph(got, want)
    assert all(t.device.type == "cuda" for t in (got["state"], got["obj_state_raw"], got["state_mask"], got["fps_idx_list"][0]))


def test_construct_graph_with_numpy_s_generator_and_its_late_refusal(dev):
    import adaptigraph_amd as ag
    clouds = _objects((9000, 300), np.random.default_rng(3))
    np.random.seed(11)
    draws = []
    for c in clouds:
        a = np.random.randint(0, len(c))
        draws.append((a, np.random.randint(100)))
    np.random.seed(11)
    _same_graph(ag.construct_graph(clouds, 0.8, device=dev), CR.construct_graph(clouds, 0.8, draws))
    with pytest.raises(ValueError, match="exceed max_nobj 100"):       # radius 0 keeps 100 points of each object
        ag.construct_graph(clouds, 0.0, device=dev, draws=draws)


def test_state_cur_from_points_equals_the_restatement(dev):
    import adaptigraph_amd as ag
    rng = np.random.default_rng(4)
    points = (rng.normal(size=(20_000, 3)) * [0.03, 0.02, 0.003] + [0.3, -0.1, 0.02])   # float64 metres, as np.array(pcd.points)
    draws = [(12_345, 67)]
    obj_kps = CR.transform(points, 10)
    want = CR.construct_graph(obj_kps, 0.2, draws)
    state_cur, cloud = ag.state_cur_from_points(points, 10, device=dev, draws=draws)
    assert state_cur.dtype == torch.float32 and state_cur.device.type == "cuda" and cloud.device.type == "cuda"
    assert np.array_equal(cloud.cpu().numpy().view(np.uint32), obj_kps.view(np.uint32))
    assert 1 < len(want["obj_state_raw"]) < 100
    assert np.array_equal(state_cur.cpu().numpy().view(np.uint32), want["obj_state_raw"].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 5. workspace
def test_a_second_call_of_the_same_size_allocates_nothing(dev):
    import adaptigraph_amd as ag
    rng = np.random.default_rng(9)
    eng = ag.default_engine(dev)
    cases = [(_cloud("rand", 40_000, rng), 1, 0.3, 2), (_cloud("rand", 100, rng), 1, 0.3, 2)]
    first = _run(dev, cases, 100, 40_000)
    before = eng.alloc_counts()
    again = _run(dev, cases, 100, 40_000)
    small = _run(dev, cases[1:], 100, 100)                   # and a smaller call lives in what is there
    assert eng.alloc_counts() == before
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    assert np.array_equal(small[0][0], first[0][1])
