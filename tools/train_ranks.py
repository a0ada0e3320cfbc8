"""Data-parallel TrainStep on a training fixture (tests/golden/train_*.npz): every rank builds TrainStep from the fixture's
weights, takes its contiguous shard of the fixture's graphs and runs AG_TRAIN_STEPS optimiser steps with total = all graphs;
apply() all-reduces gradients, loss vector and overflow word over the default process group.  Prints one JSON line (rank 0) with,
per rank: the loss of every step, the SHA-256 of the 22 weights before the first and after every step, the applied-step count and
whether check() raised.

  python tools/train_ranks.py                                              (one process, no group: plain TrainStep.step)
  AG_BENCH_FORCE_DIST=1 python tools/train_ranks.py                        (world of one on nccl = RCCL)
  AG_BENCH_SHARE_GPU=1 python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P \
        tools/train_ranks.py                                               (two ranks on one GPU, gloo)
env: AG_TRAIN_FIXTURE (train_rope.npz), AG_TRAIN_STEPS (3), AG_TRAIN_PARTS (1: micro-batches per rank and step),
AG_TRAIN_OVERFLOW_RANK (-1: that rank's LAST step gets a max_edges below its largest graph), AG_TRAIN_DUMP (file: rank 0 saves
the 22 gradients of step 1 there), AG_TRAIN_SPIN (1: one more step behind a ~100 ms spin kernel, reports whether the calls
returned while it ran), AG_BENCH_BACKEND (gloo when AG_BENCH_SHARE_GPU=1, else nccl).
Diagnostic / test driver (tests/test_gpu_train_ranks.py)."""
import hashlib, json, os, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
CFG = dict(verbose=False, nf_particle=150, nf_relation=150, nf_effect=150, nf_physics=10, attr_dim=2, state_dim=0, offset_dim=0,
           action_dim=3, density_dim=0, pstep=3, sequence_len=4, rel_particle_dim=0, rel_attr_dim=2, rel_group_dim=1,
           rel_distance_dim=3, rel_density_dim=0)


def shard_data(f, idx, dev):
    """The dict TrainStep takes, for the graphs `idx` of a fixture."""
    from adaptigraph_amd.graph import EdgeList
    N = f["attrs"].shape[1]
    off = np.concatenate([[0], np.cumsum(f["n_edges"])])
    cap = max(1, int(max(f["n_edges"][b] for b in idx)))
    recv, send = np.zeros((len(idx), cap), np.int32), np.zeros((len(idx), cap), np.int32)
    row_ptr = np.zeros((len(idx), N + 1), np.int32)
    for i, b in enumerate(idx):
        r, s = f["recv"][off[b]:off[b + 1]], f["send"][off[b]:off[b + 1]]
        recv[i, :len(r)], send[i, :len(s)] = r, s
        row_ptr[i, 1:] = np.cumsum(np.bincount(r, minlength=N))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    tf = lambda a: t(np.asarray(a, np.float32))                        # noqa: E731
    d = {k: tf(f[k][idx]) for k in ("state", "attrs", "p_instance", "action", "state_future", "eef_future", "action_future")}
    d["phys_physics_param"] = tf(f["physics_param"][idx])
    d["edges"] = EdgeList(t(recv), t(send), t(row_ptr), t(f["n_edges"][idx].astype(np.int32)), N)
    return d, int(f["n_edges"][idx].max())


def weights_sha(ts):
    h = hashlib.sha256()
    for w in ts.w:
        h.update(w.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def main():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    share = os.environ.get("AG_BENCH_SHARE_GPU") == "1"
    if share:
        local %= torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import torch.distributed as dist
    dist_on = world > 1 or os.environ.get("AG_BENCH_FORCE_DIST") == "1"
    backend = None
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        backend = os.environ.get("AG_BENCH_BACKEND", "gloo" if share else "nccl")
        kw = dict(rank=rank, world_size=world)
        if backend == "nccl":
            kw["device_id"] = dev
        dist.init_process_group(backend, **kw)
    import adaptigraph_amd as ag
    import train_restate as TR
    f = TR.load_fixture(os.environ.get("AG_TRAIN_FIXTURE", "train_rope.npz"))
    steps = int(os.environ.get("AG_TRAIN_STEPS", "3"))
    n_parts = int(os.environ.get("AG_TRAIN_PARTS", "1"))
    bad_rank = int(os.environ.get("AG_TRAIN_OVERFLOW_RANK", "-1"))
    B = f["attrs"].shape[0]
    mine = list(range(rank * B // world, (rank + 1) * B // world))
    material = "rope"
    model = ag.DynamicsPredictor(dict(CFG, pstep=int(f["pstep"])),
                                 {"material_index": {material: 0}, material: {"physics_params": [{"name": "p", "use": True}]}},
                                 {"n_his": f["state"].shape[1], "materials": [material]}, dev)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in TR.fixture_weights(f).items()})
    ts = ag.TrainStep(model.to(dev), lr=0.001, n_future=int(f["n_future"]), group=True if dist_on else None,
                      global_rows=B if dist_on else None)
    cuts = [mine[i * len(mine) // n_parts:(i + 1) * len(mine) // n_parts] for i in range(n_parts)]
    parts = [shard_data(f, idx, dev) for idx in cuts if idx]

    def one_step(bounds):
        if not dist_on and len(parts) == 1:
            return ts.step(parts[0][0], max_edges=bounds[0])
        return ts.step_parts([p[0] for p in parts], max_edges=bounds)
    losses, shas = [], [weights_sha(ts)]
    for s in range(steps):
        bounds = [p[1] for p in parts]
        if rank == bad_rank and s == steps - 1:
            bounds[-1] -= 5
        losses.append(float(one_step(bounds)))
        shas.append(weights_sha(ts))
        if s == 0 and rank == 0 and os.environ.get("AG_TRAIN_DUMP"):
            np.savez(os.environ["AG_TRAIN_DUMP"], **{k: g.cpu().numpy() for k, g in zip(TR.KEYS, ts.grad)})
    raised = False
    try:
        ts.check()
    except Exception as e:
        raised = str(e) == "Exceeds max dims"
        if not raised:
            raise
    out = {"rank": rank, "graphs": mine, "losses": losses, "weights_sha256": shas, "applied_steps": int(ts._status[1]),
           "host_step_counter": ts._step, "check_raised": raised}
    if os.environ.get("AG_TRAIN_SPIN") == "1":
        bounds = [p[1] for p in parts]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one_step(bounds)
        T = time.perf_counter() - t0                               # host time of a step's enqueues on an idle stream
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(10_000_000)
        e1.record()
        torch.cuda.synchronize()
        want_ms = max(100.0, 4e3 * T)
        done = torch.cuda.Event()
        torch.cuda._sleep(int(want_ms / (e0.elapsed_time(e1) / 10_000_000)))
        done.record()
        one_step(bounds)
        out["returned_while_busy"] = not done.query()
        out["spin_ms"], out["host_ms_of_a_step"] = want_ms, T * 1e3
        torch.cuda.synchronize()
    per = [out]
    if dist_on:
        per = [None] * world
        dist.all_gather_object(per, out)
    if rank == 0:
        print(json.dumps({"tool": "train_ranks", "world": world, "backend": backend, "steps": steps, "parts_per_rank": len(parts),
                          "ranks": per}))
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
