"""GPU checks (-m gpu) of ag_fps_cloud_grid and the *_grid functions of adaptigraph_amd.perception: the cell-pruned sampler against
ag_fps_cloud where both apply, against tests/dataset_restate.py's brute-force sweeps beyond 1024 samples, for forced cell counts
(the partition never enters the result), on non-finite coordinates, and construct_graph_grid / state_cur_from_points_grid against
tests/cloud_restate.py.  Every check is an equality of integer indices, counts or the bits of gathered fp32 values."""
import numpy as np
import pytest
import torch

import cloud_restate as CR
import dataset_restate as DR
from adaptigraph_amd.perception import CLOUD_MAX_POINTS, CLOUD_SWITCH_POINTS as S, CLOUD_WG as W, GRID_MAX_NOBJ
from oracle import adaptigraph_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ clouds
def _cloud(kind, n, rng):                                    # tests/test_gpu_dataset.py's generator
    if kind == "dup":
        return np.repeat(rng.normal(size=(1, 3)), n, 0).astype(np.float32)
    if kind == "grid":                                       # many exactly equal distances: ties everywhere
        g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
        return (g[np.arange(n) % 1000] * 0.125).astype(np.float32)
    return (rng.normal(size=(n, 3)) * [1.0, 0.1, 0.6]).astype(np.float32)


def _fps_cases(sizes, rng, max_nobj):
    """(cloud, fps_start, radius, rad_start) per sample: every size with its starts at both ends, radius 0 (every stage-1 point),
    a radius above the cloud (one point) and a usual one, a grid and a repeated point."""
    out = []
    for n in sizes:
        n1 = min(n, max_nobj)
        c = _cloud("rand", n, rng)
        out += [(c, 0, 0.3, n1 - 1), (c, n - 1, 0.0, 0), (c, n // 2, 100.0, n1 // 2), (_cloud("grid", n, rng), n - 1, 0.26, 0),
                (_cloud("dup", n, rng), n // 3, 0.0, n1 - 1)]
    return out


def _kind(kind, n, rng):
    if kind == "flat":                                       # zero y extent
        c = _cloud("rand", n, rng)
        c[:, 1] = F32(0.25)
        return c
    if kind == "lattice":                                    # pitch 0.05: ties everywhere
        side = int(round(n ** 0.5))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)
        return np.stack([g[:, 0] * 0.05, np.zeros(n), g[:, 1] * 0.05], 1).astype(F32)
    if kind == "dup4":                                       # every point four times
        return np.tile(_cloud("rand", n // 4, rng), (4, 1))
    return _cloud("dup" if kind == "repeat" else "rand", n, rng)


def _run(dev, cases, max_nobj, max_pts, cells=None, fn=None):
    """cases: (cloud, fps_start, radius, rad_start) per cloud of one launch of fps_cloud_grid(cells=...), or of `fn`."""
    from adaptigraph_amd.perception import fps_cloud_grid
    sizes = [len(c[0]) for c in cases]
    off = np.concatenate([[0], np.cumsum(sizes)])
    pos = torch.from_numpy(np.concatenate([c[0] for c in cases])).to(dev)
    tab = torch.from_numpy(np.stack([off[:-1], sizes], 1).astype(np.int64)).to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)   # noqa: E731
    args = (pos, tab[:, 0], tab[:, 1], i32([c[1] for c in cases]), torch.tensor([c[2] for c in cases], dtype=torch.float32, device=dev),
            i32([c[3] for c in cases]), max_nobj, max_pts)
    idx, n_obj = fn(*args) if fn else fps_cloud_grid(*args, cells=cells)
    return idx.cpu().numpy(), n_obj.cpu().numpy()


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])


_ref = {}                                                    # references are computed once and shared, never changed


def _cached(key, make):
    if key not in _ref:
        _ref[key] = make()
    return _ref[key]


# ------------------------------------------------------------------------------------------------ 1. against ag_fps_cloud
SIZE_LISTS = [((1, 2, W - 1, W, W + 1), 100), ((8192, 8193, S - 1, S, S + 1), 100), ((100_000,), 100), ((CLOUD_MAX_POINTS,), 16),
              ((1500,), 1024)]


@pytest.mark.parametrize("cells", [1, 8, None])
@pytest.mark.parametrize("which", range(len(SIZE_LISTS)))
def test_equals_fps_cloud_where_both_apply(dev, which, cells):
    """tests/test_gpu_cloud_fps.py's sizes and kinds: equal outputs, padding included, for the brute-force sweep through the same
    code (cells = 1), a forced count and the default policy."""
    from adaptigraph_amd.perception import fps_cloud
    sizes, max_nobj = SIZE_LISTS[which]
    cases = _fps_cases(sizes, np.random.default_rng(len(sizes) + max_nobj), max_nobj)
    want = _cached(("cloud", which), lambda: _run(dev, cases, max_nobj, max(sizes), fn=fps_cloud))
    assert _same(_run(dev, cases, max_nobj, max(sizes), cells), want)


def _mix(rng):
    return [(_cloud("rand", n, rng), s, r, rs) for n, s, r, rs in
            [(0, 0, 0.2, 0), (1, 0, 0.2, 0), (300, 299, 0.25, 99), (8193, 17, 0.3, 5), (70_000, 69_999, 0.2, 0)]]


@pytest.mark.parametrize("cells", [1, 8, None])
def test_one_launch_of_an_empty_a_one_point_and_larger_clouds(dev, cells):
    from adaptigraph_amd.perception import fps_cloud
    cases = _mix(np.random.default_rng(7))
    want = _cached("mix", lambda: _run(dev, cases, 100, 80_000, fn=fps_cloud))
    got = _run(dev, cases, 100, 80_000, cells)
    assert _same(got, want) and got[1][0] == 0 and (got[0][0] == -1).all()


def test_starts_out_of_range_are_clamped_and_a_count_above_max_pts_is_truncated(dev):
    from adaptigraph_amd.perception import fps_cloud
    c = _cloud("rand", 5000, np.random.default_rng(8))
    cases = [(c, -3, 0.3, 4000), (c, 10**6, 0.3, -1)]
    assert _same(_run(dev, cases, 100, 5000), _run(dev, cases, 100, 5000, fn=fps_cloud))
    assert _same(_run(dev, [(c, 4999, 0.3, 0)], 100, 3000), _run(dev, [(c, 4999, 0.3, 0)], 100, 3000, fn=fps_cloud))
    idx, n_obj = _run(dev, [(c, 10**6, 0.05, -1)], 1500, 3000)                       # and beyond the old limit
    want = DR.fps_indices(c[:3000], 1500, 2999, 0.05, 0)
    assert n_obj[0] == len(want) and np.array_equal(idx[0, :len(want)], want) and (idx[0, len(want):] == -1).all()


# ------------------------------------------------------------------------------------------------ 2. beyond 1024 samples
BEYOND = [("rand", 3000, 1025, 0.05), ("rand", 1025, 1025, 0.0), ("rand", 700, 1025, 0.02), ("flat", 5000, 2049, 0.03),
          ("lattice", 4900, 2049, 0.05), ("lattice", 4900, 2049, 0.0500001), ("dup4", 6000, 1500, 0.01), ("repeat", 1500, 1025, 0.2),
          ("rand", 50_000, 2049, 0.02), ("rand", 100_000, 4096, 0.01), ("rand", CLOUD_MAX_POINTS, 16, 0.3)]


def _beyond(which):
    kind, n, max_nobj, radius = BEYOND[which]
    rng = np.random.default_rng(1000 + which)
    c = _kind(kind, n, rng)
    case = (c, int(rng.integers(n)), radius, int(rng.integers(min(n, max_nobj))))
    return case, max_nobj, _cached(("beyond", which), lambda: DR.fps_indices(c, max_nobj, case[1], radius, case[3]))


def _check(got, b, want, max_nobj):
    idx, n_obj = got
    assert n_obj[b] == len(want), (b, int(n_obj[b]), len(want))
    assert np.array_equal(idx[b, :len(want)], want) and (idx[b, len(want):] == -1).all() and idx.shape[1] == max_nobj


@pytest.mark.parametrize("which", range(len(BEYOND)))
def test_beyond_the_old_limit_equals_the_brute_force_sweep(dev, which):
    case, max_nobj, want = _beyond(which)
    if BEYOND[which][:3] == ("rand", 700, 1025):
        assert len(want) <= 700 and len(set(want.tolist())) == len(want)             # n < max_nobj: stage 1 selects every point
    _check(_run(dev, [case], max_nobj, len(case[0])), 0, want, max_nobj)


@pytest.mark.parametrize("cells", [1, 2, 64])
@pytest.mark.parametrize("which", range(4))
def test_the_cell_count_never_enters_the_result(dev, which, cells):
    case, max_nobj, want = _beyond(which)
    _check(_run(dev, [case], max_nobj, len(case[0]), cells), 0, want, max_nobj)


def test_the_lattice_equals_the_restatement_below_the_old_limit_too(dev):
    """Stage 2's square root is correctly rounded here, as numpy's is: on the lattice of pitch 0.05, where distances lie within an
    ulp of each other and of the radius, the new path follows the restatement at 1024 samples as well."""
    rng = np.random.default_rng(12)
    c = _kind("lattice", 4900, rng)
    for radius in (0.05, 0.0500001):
        _check(_run(dev, [(c, 2450, radius, 5)], 1024, 4900), 0, DR.fps_indices(c, 1024, 2450, radius, 5), 1024)


# ------------------------------------------------------------------------------------------------ 3. one launch, four kinds
def test_four_clouds_of_different_kinds_and_sizes_in_one_launch(dev):
    rng = np.random.default_rng(33)
    cases = [(_kind("rand", 3000, rng), 2999, 0.04, 7), (_kind("flat", 5000, rng), 0, 0.03, 1199), (_kind("lattice", 4900, rng), 2450, 0.05, 3),
             (_kind("repeat", 1500, rng), 11, 0.0, 1199)]
    got = _run(dev, cases, 1200, 6000)
    for b, (c, s, r, rs) in enumerate(cases):
        _check(got, b, DR.fps_indices(c, 1200, s, r, rs), 1200)


# ------------------------------------------------------------------------------------------------ 4. non-finite coordinates
def test_non_finite_coordinates_are_swept_like_the_brute_force_sweep(dev):
    """The rule is "equal to the brute-force sweep": such a point's minimum never drops (md > d is false for a NaN or infinite d),
    so from the pick that reaches the lowest such index on it is chosen again and again - by fps_cloud, by cells = 1 and by any
    partition alike."""
    from adaptigraph_amd.perception import fps_cloud
    c = _cloud("rand", 3000, np.random.default_rng(44))
    c[1234, 1] = np.nan
    c[77, 2] = np.inf
    case = [(c, 5, 0.05, 3)]
    want = _run(dev, case, 100, 3000, fn=fps_cloud)
    for cells in (1, 8, None):
        assert _same(_run(dev, case, 100, 3000, cells), want), cells
    want = _run(dev, case, 1025, 3000, 1)
    for cells in (8, 64, None):
        assert _same(_run(dev, case, 1025, 3000, cells), want), cells


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_above_the_limits_is_refused_before_anything_is_allocated_or_enqueued(dev):
    import adaptigraph_amd as ag
    from adaptigraph_amd import _lib
    z = torch.zeros(8, dtype=torch.int64, device=dev)
    i32 = z[:1].int()
    with pytest.raises(NotImplementedError, match=str(CLOUD_MAX_POINTS)):
        ag.fps_cloud_grid(torch.zeros(4, 3, device=dev), z[:1], z[:1], i32, z[:1].float(), i32, 100, CLOUD_MAX_POINTS + 1)
    with pytest.raises(NotImplementedError, match=str(GRID_MAX_NOBJ)):
        ag.fps_cloud_grid(torch.zeros(4, 3, device=dev), z[:1], z[:1], i32, z[:1].float(), i32, GRID_MAX_NOBJ + 1, 4)
    eng = ag.default_engine(dev)
    lib = _lib.load_cells()
    out = torch.full((8,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    before = eng.alloc_counts()
    p = z.data_ptr()
    for max_nobj, max_pts, limit in ((100, CLOUD_MAX_POINTS + 1, CLOUD_MAX_POINTS), (GRID_MAX_NOBJ + 1, 4, GRID_MAX_NOBJ)):
        rc = lib.ag_fps_cloud_grid(eng.ctx, None, p, p, p, 1, p, p, p, 1, max_nobj, max_pts, 0, out.data_ptr(), out.data_ptr())
        assert rc == _lib.AG_ERR_UNSUPPORTED and str(limit) in eng.lib.ag_last_error(eng.ctx).decode()
    assert lib.ag_fps_cloud_grid(eng.ctx, None, p, p, p, 1, p, p, p, 1, 100, 4, 3, out.data_ptr(), out.data_ptr()) == _lib.AG_ERR_INVALID
    torch.cuda.synchronize(dev)
    assert eng.alloc_counts() == before and (out == 7).all()


# ------------------------------------------------------------------------------------------------ 6. construct_graph_grid
def _objects(sizes, rng):
    return [((rng.normal(size=(n, 3)) * [1.0, 0.1, 0.6]) + [4.0 * j, 0, 0]).astype(np.float32) for j, n in enumerate(sizes)]


def _same_graph(got, want):
    for k in ("state", "obj_state", "obj_state_raw", "eef_state"):
        g = got[k].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == want[k].shape, (k, g.shape, want[k].shape)
        assert np.array_equal(g.view(np.uint32), want[k].view(np.uint32)), k
    for k in ("state_mask", "eef_mask"):
        g = got[k].cpu().numpy()
        assert got[k].dtype == torch.bool and np.array_equal(g, np.asarray(want[k].cpu() if torch.is_tensor(want[k]) else want[k])), k
    assert len(got["fps_idx_list"]) == len(want["fps_idx_list"])
    for g, w in zip(got["fps_idx_list"], want["fps_idx_list"]):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w.cpu().numpy() if torch.is_tensor(w) else w)


def test_construct_graph_grid_equals_the_restatement_and_construct_graph(dev):
    import adaptigraph_amd as ag
    rng = np.random.default_rng(6)
    clouds = _objects((6000, 2500), rng)
    eef = rng.normal(size=(3, 3)).astype(np.float32)
    draws = [(int(rng.integers(6000)), int(rng.integers(5000))), (int(rng.integers(2500)), int(rng.integers(2500)))]
    want = CR.construct_graph(clouds, 0.07, draws, max_nobj=5000, eef_kps=eef)
    assert 1024 < len(want["obj_state"]) <= 5000 and all(len(i) > 100 for i in want["fps_idx_list"])
    got = ag.construct_graph_grid(clouds, 0.07, max_nobj=5000, eef_kps=eef, device=dev, draws=draws)
    _same_graph(got, want)
    assert got["state"].shape == (5008, 3) and got["state"].device.type == "cuda"
    draws = [(a, b % 100) for a, b in draws]                                          # where construct_graph applies: itself
    old = ag.construct_graph(clouds, 0.8, eef_kps=eef, device=dev, draws=draws)
    new = ag.construct_graph_grid(clouds, 0.8, eef_kps=eef, device=dev, draws=draws)
    _same_graph(new, {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in old.items()})
    with pytest.raises(ValueError, match="exceed max_nobj 5000"):                    # the late refusal stays: 5000 + 2500 points kept
        ag.construct_graph_grid(clouds, 0.0, max_nobj=5000, device=dev, draws=[(0, 0), (0, 0)])


def test_state_cur_from_points_grid_equals_the_restatement(dev):
    import adaptigraph_amd as ag
    rng = np.random.default_rng(4)
    points = (rng.normal(size=(20_000, 3)) * [0.03, 0.02, 0.003] + [0.3, -0.1, 0.02])   # float64 metres, as np.array(pcd.points)
    draws = [(12_345, 4000)]
    obj_kps = CR.transform(points, 10)
    want = CR.construct_graph(obj_kps, 0.03, draws, max_nobj=4097)
    assert 1024 < len(want["obj_state_raw"]) < 4097
    state_cur, cloud = ag.state_cur_from_points_grid(points, 10, fps_radius=0.03, max_nobj=4097, device=dev, draws=draws)
    assert state_cur.dtype == torch.float32 and state_cur.device.type == "cuda" and cloud.device.type == "cuda"
    assert np.array_equal(cloud.cpu().numpy().view(np.uint32), obj_kps.view(np.uint32))
    assert np.array_equal(state_cur.cpu().numpy().view(np.uint32), want["obj_state_raw"].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 7. from the cloud to the graph
def test_a_cloud_becomes_a_graph_of_more_than_4096_particles(dev):
    """A 90 x 90 jittered sheet -> construct_graph_grid -> construct_edges_cells: the state and the edge lists equal what the numpy
    restatement and the oracle's builder give."""
    import adaptigraph_amd as ag
    rng = np.random.default_rng(9)
    g = np.stack(np.meshgrid(np.arange(90), np.arange(90), indexing="ij"), -1).reshape(-1, 2) * 0.02
    sheet = np.stack([g[:, 0], np.zeros(len(g)), g[:, 1]], 1) + rng.normal(size=(len(g), 3)) * [0.004, 0.001, 0.004]
    sheet = sheet.astype(np.float32)
    eef = np.array([[0.9, 0.05, 0.9], [0.2, 0.05, 0.3]], np.float32)
    draws, radius, max_nobj = [(4321, 17)], 0.019, 4200
    want = CR.construct_graph(sheet, radius, draws, max_nobj=max_nobj, eef_kps=eef)
    K = len(want["obj_state"])
    assert 4096 < K < max_nobj, K                            # the radius was chosen on the CPU
    got = ag.construct_graph_grid(sheet, radius, max_nobj=max_nobj, eef_kps=eef, device=dev, draws=draws)
    _same_graph(got, want)
    tool = got["eef_mask"][None]
    el = ag.construct_edges_cells(got["state"][None], 0.03, got["state_mask"][None], tool, topk=5, connect_tools_all=False)
    recv, send = O.construct_edges_single(want["state"], 0.03, want["state_mask"], want["eef_mask"], 5, False)
    n = int(el.n_edges[0])
    assert n == len(recv) and n > K
    assert np.array_equal(el.recv[0, :n].cpu().numpy(), recv) and np.array_equal(el.send[0, :n].cpu().numpy(), send)
