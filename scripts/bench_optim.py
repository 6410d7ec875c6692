#!/usr/bin/env python3
"""Times the optimizer updates over the two flat parameter tensors of a field pair (one JSON line, also written to --out):

    python scripts/bench_optim.py [--rounds 7] [--steps 50] [--warmup 10] [--out profiles/optim_bench.json]

  flat_sgd     mnrf_sgd_step    beside   torch_sgd_fused      torch.optim.SGD(fused=True)
  flat_radam   mnrf_radam_step  beside   torch_radam_foreach  torch.optim.RAdam(foreach=True) (torch has no fused RAdam)
  flat_adam    mnrf_adam_step   beside   torch_adam_fused     torch.optim.Adam(fused=True)
each over the same two tensors of a MirrorNeRF's parameter count (595 k elements) with the same gradients.  Microseconds per
step and model: the time between two torch.cuda.Event records around `steps` consecutive steps of both tensors, divided by
2 * steps -- launches with the gaps between them, as a training step meets them, not the kernels alone.  The six routes take
turns within a round; the figure is the median of the rounds, with the extremes."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    a = ap.parse_args(argv)
    import torch
    import mirror_nerf_amd as M
    from mirror_nerf_amd import _lib, dist
    dev = torch.device("cuda", 0)
    n = dist._field_layout(M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True))[1]
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    grads = [torch.randn(n, device=dev, generator=gen) * 1e-3 for _ in range(2)]
    L, p = _lib.lib(), _lib.ptr

    def flat(entry, n_state, scalars):
        ps = [torch.randn(n, device=dev, generator=gen) * 0.1 for _ in range(2)]
        state = [[torch.zeros(n, device=dev) for _ in range(n_state)] for _ in range(2)]
        skipped = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2)]
        fn, count = getattr(L, entry), [0]

        def step():
            count[0] += 1
            for q, g, st, sk in zip(ps, grads, state, skipped):
                _lib.check(fn(p(q), p(g), *[p(t) for t in st], n, *scalars, count[0], p(sk), None, None, _lib.stream()), entry)
        return step

    def torch_opt(make):
        ps = [torch.nn.Parameter(torch.randn(n, device=dev, generator=gen) * 0.1) for _ in range(2)]
        opt = make(ps)
        for q, g in zip(ps, grads):
            q.grad = g
        return opt.step

    routes = {
        "flat_sgd": flat("mnrf_sgd_step", 1, (5e-4, 0.9, 0.0)),
        "torch_sgd_fused": torch_opt(lambda ps: torch.optim.SGD(ps, lr=5e-4, momentum=0.9, fused=True)),
        "flat_radam": flat("mnrf_radam_step", 2, (5e-4, 0.9, 0.999, 1e-8, 0.0)),
        "torch_radam_foreach": torch_opt(lambda ps: torch.optim.RAdam(ps, lr=5e-4, foreach=True)),
        "flat_adam": flat("mnrf_adam_step", 2, (5e-4, 0.9, 0.999, 1e-8, 0.0)),
        "torch_adam_fused": torch_opt(lambda ps: torch.optim.Adam(ps, lr=5e-4, fused=True)),
    }
    for step in routes.values():
        for _ in range(a.warmup):
            step()
    torch.cuda.synchronize()
    us = {k: [] for k in routes}
    for _ in range(a.rounds):
        for name, step in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / (2 * a.steps))
    line = {"what": "optimizer update, microseconds per step and model (device events around consecutive steps of two tensors)",
            "elements_per_model": n, "rounds": a.rounds, "steps_per_round": a.steps, "device": torch.cuda.get_device_name(0),
            "torch": torch.__version__,
            "us_per_step_per_model": {k: round(statistics.median(v), 3) for k, v in us.items()},
            "minmax_us": {k: [round(min(v), 3), round(max(v), 3)] for k, v in us.items()}}
    text = json.dumps(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
