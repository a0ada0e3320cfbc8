"""CPU checks of the Earth-mover loss: the numpy restatement (tests/emd_restate.py) against scipy.optimize.linear_sum_assignment and
against the reference's own values, gradients and assignments (tests/golden/emd.npz, train_emd_rope.npz), the conditions the
fixtures were generated under, the seeded cases of the GPU tests, LossSpec's Earth-mover term, and the boundary's header."""
import os
import re

import numpy as np
import pytest
import torch

import emd_restate as ER
import train_restate as TR
from test_train import grad_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (2, 2, 2), (3, 7, 5), (3, 5, 7), (2, 64, 64), (2, 65, 70), (2, 100, 100), (1, 257, 300), (2, 9, 9), (1, 48, 48)]
CHAIN = 9
# seeded random cases of tests/test_gpu_emd.py, (B, N, M, seed): N != M both ways, B up to 4, sizes on either side of 64 and 256.
# The seeds were chosen here on the CPU so that every graph has gap >= 1e-5 (test_seeded_cases_meet_their_gap_bar holds them to it)
SEEDED = [(4, 5, 9, 0), (3, 9, 5, 0), (3, 33, 33, 0), (2, 63, 66, 0), (2, 66, 63, 0), (2, 64, 64, 0), (1, 255, 258, 1), (1, 258, 255, 1),
          (1, 256, 256, 0)]
SEEDED_GAP = 1e-5


def emd_cases():
    f = TR.load_fixture("emd.npz")
    return [{key.split("::", 1)[1]: f[key] for key in f if key.startswith(f"c{k}::")} for k in range(int(f["n_cases"]))]


def fixture_losses(f):
    return [(str(n), float(w)) for n, w in zip(f["loss_names"], f["loss_weights"])]


def seeded_clouds(B, N, M, seed):
    rng = np.random.default_rng([seed, B, N, M])
    x = rng.normal(0, 0.3, (B, N, 3)).astype(np.float32)
    y = (x[:, rng.integers(0, N, M)] + rng.normal(0, 0.1, (B, M, 3))).astype(np.float32)
    return x, y


def test_fixture_cases_are_the_stated_shapes():
    cases = emd_cases()
    assert [(c["x"].shape[0], c["x"].shape[1], c["y"].shape[1]) for c in cases] == SHAPES
    c = cases[8]
    assert np.array_equal(c["x"][0, 2], c["y"][0, 4])                       # the coincident pair, and it is matched
    assert c["ind2"][0][list(c["ind1"][0]).index(2)] == 4
    for c, (B, N, M) in zip(cases, SHAPES):
        K = min(N, M)
        assert c["ind1"].shape == c["ind2"].shape == (B, K) and c["gap"].shape == (B,)
        assert (np.diff(c["ind1"], axis=1) > 0).all()                       # ascending, as linear_sum_assignment returns it
        assert all(len(set(r.tolist())) == K for r in c["ind2"])            # one-to-one


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_restatement_equals_scipy_on_the_fixtures(k):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    c = emd_cases()[k]
    for b in range(c["x"].shape[0]):
        for dtype in (np.float32, np.float64):
            cost = ER.cost_matrix(c["x"][b], c["y"][b], dtype)
            i1, i2, _ = ER.solve(cost)
            r1, r2 = lsa(cost)
            assert np.array_equal(i1, r1) and np.array_equal(i2, r2), (k, b, dtype)
            assert np.array_equal(i1, c["ind1"][b]) and np.array_equal(i2, c["ind2"][b])     # and what the reference's run picked


@pytest.mark.parametrize("n,m", [(1, 1), (1, 4), (4, 1), (2, 2), (3, 8), (8, 3), (17, 17), (40, 55), (55, 40), (90, 90)])
def test_restatement_equals_scipy_on_random_matrices(n, m):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for seed in range(4):
        cost = np.random.default_rng([seed, n, m]).random((n, m))
        i1, i2, steps = ER.solve(cost)
        r1, r2 = lsa(cost)
        assert np.array_equal(i1, r1) and np.array_equal(i2, r2)
        assert steps.shape == (min(n, m),) and (steps >= 1).all() and (steps <= np.arange(1, min(n, m) + 1)).all()


def test_restatement_equals_scipy_on_the_seeded_cases():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for B, N, M, seed in SEEDED:
        x, y = seeded_clouds(B, N, M, seed)
        for b in range(B):
            cost = ER.cost_matrix(x[b], y[b], np.float32)
            i1, i2, _ = ER.solve(cost)
            r1, r2 = lsa(cost)
            assert np.array_equal(i1, r1) and np.array_equal(i2, r2), (B, N, M, b)


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_restatement_reproduces_values_gradients_and_gaps(k):
    c = emd_cases()[k]
    v, g = ER.value_and_grad(c["x"], c["y"])
    ref, g_ref = float(c["emd"]), c["g_emd"]
    assert abs(v - ref) <= 1e-5 * abs(ref), (v, ref)
    assert abs(v - float(c["emd_64"])) <= 1e-12 * abs(ref)
    assert np.isfinite(g).all()
    assert np.abs(g - g_ref).max() <= 1e-4 * np.abs(g_ref).max() + 1e-7, np.abs(g - g_ref).max()
    assert np.allclose(ER.batch_gaps(c["x"], c["y"]), c["gap"], rtol=0, atol=1e-12)
    B, N, M = SHAPES[k]
    matched = np.zeros((B, N), bool)
    matched[np.arange(B)[:, None], c["ind1"]] = True
    assert (g_ref[~matched] == 0).all() and (~matched).sum() == B * max(0, N - M)      # unmatched x rows: zero gradient
    if k == 8:
        assert (g_ref[0, 2] == 0).all() and (g[0, 2] == 0).all()            # zero distance, zero gradient


def test_fixtures_meet_the_conditions():
    f = TR.load_fixture("emd.npz")
    assert float(f["gap_bar"]) == 1e-4
    for k, c in enumerate(emd_cases()):
        B, N, M = SHAPES[k]
        assert (c["gap"] >= 1e-4).all(), (k, c["gap"])
        i32, i64 = ER.assignment(c["x"], c["y"], np.float32), ER.assignment(c["x"], c["y"], np.float64)
        assert all(np.array_equal(a, b) for a, b in zip(i32, i64))          # fp32 and float64 costs pick the same assignment
        costs = [ER.cost_matrix(a, b) for a, b in zip(c["x"], c["y"])]
        if min(N, M) >= 5:
            assert all(ER.shortcuts_fail(cm) for cm in costs), k
        if k == 1:                                                          # (2,2,2): both x points are nearest to the same y point
            assert all((cm.argmin(1) == cm.argmin(1)[0]).all() for cm in costs)
            assert all(not np.array_equal(ER.greedy(cm), ER.solve(cm)[1]) for cm in costs)
        if k == CHAIN:
            steps = ER.solve(costs[0])[2]
            assert steps.max() >= min(N, M) / 2, steps
    t = TR.load_fixture("train_emd_rope.npz")
    assert float(t["gap_bar"]) == 1e-4 and t["step_gaps"].shape == (int(t["n_future"]), t["attrs"].shape[0])
    assert (t["step_gaps"] >= 1e-4).all() and (t["adam_gaps"] >= 1e-4).all() and t["adam_gaps"].shape == (5,)
    assert fixture_losses(t) == [("mse", 1.0), ("earth_mover", 0.5)] and int(t["n_future"]) == 3
    assert t["attrs"].shape[:2] == (3, 41) and t["loss_terms"].shape == (3, 2) and t["adam_losses"].shape == (5,)


def test_seeded_cases_meet_their_gap_bar():
    for B, N, M, seed in SEEDED:
        x, y = seeded_clouds(B, N, M, seed)
        gaps = ER.batch_gaps(x, y)
        assert (gaps >= SEEDED_GAP).all(), (B, N, M, seed, gaps)
        i32, i64 = ER.assignment(x, y, np.float32), ER.assignment(x, y, np.float64)
        assert all(np.array_equal(a, b) for a, b in zip(i32, i64))


def test_restatement_matches_reference_training_chain():
    f = TR.load_fixture("train_emd_rope.npz")
    loss, terms, preds, g, dstate = ER.restated_chain(f, fixture_losses(f))
    assert abs(loss - float(f["loss_sum"])) <= 1e-5 * abs(float(f["loss_sum"]))
    assert abs(loss - float(f["loss_sum_64"])) <= 1e-12 * abs(loss)
    assert (np.abs(terms - f["loss_terms"]) <= 1e-5 * np.abs(f["loss_terms"])).all(), (terms, f["loss_terms"])
    fut = f["state_future"].astype(np.float64)
    for fi, p in enumerate(preds):                                          # the recorded gaps are those of the chain itself
        assert np.allclose(ER.batch_gaps(p.numpy(), fut[:, fi]), f["step_gaps"][fi], rtol=0, atol=1e-9)
    for k in TR.KEYS:
        err = np.abs(g[k] - f["g::" + k]).max()
        assert err <= grad_tol(f, k), (k, err, np.abs(f["g::" + k]).max())
    assert np.abs(dstate - f["dstate0"]).max() <= 1e-4 * np.abs(f["dstate0"]).max() + 1e-7
    assert np.abs(dstate - f["dstate0_64"]).max() <= 1e-10 * np.abs(f["dstate0_64"]).max()


# ------------------------------------------------------------------------------------------------ LossSpec: host only
def test_loss_spec_takes_the_packages_earth_mover_module():
    from adaptigraph_amd import EarthMoverLoss, earth_mover_assignment, _lib  # noqa: F401
    from adaptigraph_amd.set_losses import LossSpec
    s = LossSpec([("mse", 1), (EarthMoverLoss(), 0.5)])
    assert s.names == ["mse", "earth_mover"] and s.kinds == [0, 3] and s.weights == [1.0, 0.5] and _lib.AG_LOSS_EMD == 3
    assert not s.has_hausdorff
    for what in ("accumulate", "step_parts", "__init__(group=...)"):
        s.forbid_parts(what)                                                # a mean splits: nothing raised
    c = s.c_struct()
    assert c.n_terms == 2 and list(c.kind)[:2] == [0, 3] and list(c.weight)[:2] == [1.0, 0.5]
    assert isinstance(EarthMoverLoss(), torch.nn.Module)
    for term in ("emd", "earth_mover", "EarthMoverLoss"):                   # the strings stay refused, with the present text
        with pytest.raises(NotImplementedError, match="host step"):
            LossSpec([(term, 1)])


# ------------------------------------------------------------------------------------------------ the boundary
def test_header_declares_the_kind_and_documents_the_work_layout():
    raw = open(os.path.join(ROOT, "include", "adaptigraph_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define AG_LOSS_EMD 3\b", src)
    assert re.search(r"#define AG_ABI_VERSION 7\b", src)
    doc = " ".join(raw.split())
    assert "d_work for AG_LOSS_EMD" in doc and "match table" in doc and "status words" in doc
    from adaptigraph_amd import _lib
    assert len(_lib.EXPORTS) == 51                                          # no new export (tests/test_abi.py holds them to the header)
    common = open(os.path.join(ROOT, "adaptigraph_amd", "csrc", "ag_setloss.h")).read()
    assert re.search(r"SET_LOSS_EMD = 3\b", common) and re.search(r"EMD_MAX_MATCH = (\d+)", common).group(1) == str(_lib.EMD_MAX_MATCH)
