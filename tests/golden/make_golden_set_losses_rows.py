#!/usr/bin/env python3
"""Generate the REAL-ROWS set-loss fixture from the real reference (jhyau/AdaptiGraph): what its own ChamferLoss, HausdorffLoss and
EarthMoverLoss (src/dynamics/gnn/loss.py) and its planning-side mean_chamfer (src/planning/losses.py:12-24) give for every graph of
a PADDED batch when the graph is sliced to its real rows, x[b:b+1, :nx_b] against y[b:b+1, :ny_b] - the semantics the training
side's AG_LOSS_ROWS kinds restate for the whole batch at once.

Runs only where the reference checkout and scipy exist; the tests see only the .npz written here.

set_losses_rows.npz - batches a:: (B = 6, N = 9, M = 7, nx = [9,5,1,0,9,3], ny = [7,7,2,4,0,3]) and b:: (B = 3, N = M = 40,
nx = ny = [40,23,1]), each with x (B,N,3), y (B,M,3) (rows behind the counts are zero, as the loader pads), nx, ny, recorded (B,)
bool - graphs with both sides non-empty; the reference cannot evaluate an empty side (a min over nothing raises), so those graphs
(2 of the 6 in batch a) are left out of the recording and are covered by the rule alone - and per recorded graph, in (B, ...)
arrays whose other entries are zero (-1 for indices):
  chamfer, hausdorff, emd            fp32 values of the reference's modules on the slice
  chamfer_64, hausdorff_64, emd_64   the same modules in float64
  g_chamfer, g_hausdorff, g_emd      (B,N,3) their autograd gradients toward the slice of x
  mean_chamfer                       (B,) planning.losses.mean_chamfer of the batch's recorded graphs with the prefix masks (float64)
  ind1, ind2                         (B, min(N,M)) scipy's assignment on the reference's fp32 distance matrix of the slice
  nn_gaps (B,4), emd_gap (B,)        the conditions below, as measured

CONDITIONS (enforced here with the existing generators' own bars, imported from them; not measurements): every recorded slice's
float64 nearest-neighbour gaps (set_loss_restate.gaps, the first two entries; make_golden_set_losses.GAP_TRAIN = 1e-4), its
assignment uniqueness gap (emd_restate.gap; make_golden_emd.GAP = 1e-4), the batch-wide gap between the two largest minima per
side (set_loss_rows.qualifies), and the reference's fp32 and float64 runs pick the same assignment.  Seeds are walked from a fixed
start up to MAX_TRIES; the first that meets the conditions is stored, and nothing is written if none does.

Usage:  python tests/golden/make_golden_set_losses_rows.py
"""
import os
import sys

import numpy as np
import scipy.optimize  # noqa: F401  (loss.py says `import scipy` and uses scipy.optimize)
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import make_golden_emd as GE  # noqa: E402
import make_golden_set_losses as GS  # noqa: E402
import emd_restate as ER  # noqa: E402
import set_loss_restate as SR  # noqa: E402
import set_loss_rows as RW  # noqa: E402

OUT = HERE
MAX_TRIES = 64
NN_GAP, EMD_GAP = GS.GAP_TRAIN, GE.GAP
BATCHES = (("a", RW.BATCH_A, 700), ("b", RW.BATCH_B, 800))


def batch(tag, spec, seed, L, mean_chamfer):
    B, N, M = spec["B"], spec["N"], spec["M"]
    nx, ny = np.array(spec["nx"]), np.array(spec["ny"])
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 0.3, (B, N, 3)).astype(np.float32)
    y = (x[:, rng.integers(0, N, M)] + rng.normal(0, 0.1, (B, M, 3))).astype(np.float32)
    for b in range(B):                                          # the loader's padding: zeros behind the counts
        x[b, nx[b]:], y[b, ny[b]:] = 0, 0
    rec = (nx > 0) & (ny > 0)
    if not RW.qualifies(x, y, nx, ny):
        return None
    K = min(N, M)
    out = {"x": x, "y": y, "nx": nx.astype(np.int32), "ny": ny.astype(np.int32), "recorded": rec, "seed": np.int64(seed),
           "ind1": np.full((B, K), -1, np.int64), "ind2": np.full((B, K), -1, np.int64), "nn_gaps": np.full((B, 4), np.inf),
           "emd_gap": np.full(B, np.inf), "mean_chamfer": np.zeros(B, np.float64)}
    mods = (("chamfer", L.ChamferLoss()), ("hausdorff", L.HausdorffLoss()), ("emd", L.EarthMoverLoss()))
    for name, _ in mods:
        out[name], out[name + "_64"] = np.zeros(B, np.float32), np.zeros(B, np.float64)
        out["g_" + name] = np.zeros((B, N, 3), np.float32)
    for b in np.nonzero(rec)[0]:
        xs, ys = x[b:b + 1, :nx[b]], y[b:b + 1, :ny[b]]
        out["nn_gaps"][b] = SR.gaps(xs, ys)
        out["emd_gap"][b] = ER.batch_gaps(xs, ys)[0]
        if not (out["nn_gaps"][b, :2] >= NN_GAP).all() or not out["emd_gap"][b] >= EMD_GAP:
            return None
        i32 = GE.reference_assignment(xs, ys)
        i64 = GE.reference_assignment(xs.astype(np.float64), ys.astype(np.float64))
        if not (np.array_equal(i32[0], i64[0]) and np.array_equal(i32[1], i64[1])):
            return None
        k = i32[0].shape[1]
        out["ind1"][b, :k], out["ind2"][b, :k] = i32[0][0], i32[1][0]
        for name, mod in mods:
            xt = torch.from_numpy(xs.copy()).requires_grad_(True)
            v = mod(xt, torch.from_numpy(ys.copy()))
            v.backward()
            out[name][b] = np.float32(v.item())
            out["g_" + name][b, :nx[b]] = xt.grad.numpy()[0]
            out[name + "_64"][b] = mod(torch.from_numpy(xs).double(), torch.from_numpy(ys).double()).item()
    idx = np.nonzero(rec)[0]
    mask_x, mask_y = np.arange(N)[None] < nx[:, None], np.arange(M)[None] < ny[:, None]
    out["mean_chamfer"][idx] = mean_chamfer(torch.from_numpy(x[idx]).double(), torch.from_numpy(y[idx]).double(),
                                            torch.from_numpy(mask_x[idx]), torch.from_numpy(mask_y[idx]))
    return {f"{tag}::{k}": v for k, v in out.items()}


def main():
    sys.path.insert(0, MG.REF)
    from planning.losses import mean_chamfer
    L = GS.load_reference_losses()
    torch.set_num_threads(8)
    store = {"nn_gap_bar": np.float64(NN_GAP), "emd_gap_bar": np.float64(EMD_GAP)}
    for tag, spec, seed0 in BATCHES:
        for t in range(MAX_TRIES):
            got = batch(tag, spec, seed0 + t, L, mean_chamfer)
            if got is not None:
                break
        else:
            raise SystemExit(f"set_losses_rows batch {tag}: no seed in {MAX_TRIES} tries met the conditions; nothing written")
        store.update(got)
        rec = got[f"{tag}::recorded"]
        print(f"set_losses_rows {tag}: seed {int(got[f'{tag}::seed'])}, recorded {int(rec.sum())} of {len(rec)} graphs, "
              f"chamfer {got[f'{tag}::chamfer'][rec]}, hausdorff {got[f'{tag}::hausdorff'][rec]}, emd {got[f'{tag}::emd'][rec]}")
    path = os.path.join(OUT, "set_losses_rows.npz")
    np.savez_compressed(path, **store)
    print(f"set_losses_rows.npz: {os.path.getsize(path) / 1e6:.3f} MB")


if __name__ == "__main__":
    main()
