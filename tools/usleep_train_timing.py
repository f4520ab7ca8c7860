"""Cost of one U-Sleep training step (compute_fid.py configuration: depth 12, 2 x 3000 samples per window, fp32), one JSON line per batch size.
The variants alternate inside one process; every figure is the median of --iters calls (device events), repeated --rounds times (the spread
of the round medians is what a difference has to exceed to mean anything):

  native_step      USleep.train_step: training forward + weighted cross-entropy + backward (csrc/usleep_train.hip)
  native_forward   USleep.forward in train mode alone (csrc/usleep.hip), for scale
  torch_step       what a user would otherwise run: oracle.usleep.usleep_forward + F.cross_entropy + autograd, on the device

and the number of kernels the native step launches.  Nothing is asserted.

    python tools/usleep_train_timing.py [--iters 25] [--rounds 5] [--shapes 64x3000,8x3000]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="64x3000,8x3000")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from eegldm.metrics import USleep
    from oracle.usleep import usleep_forward
    torch.manual_seed(0)
    model = USleep(in_chans=2, sfreq=100, depth=12, with_skip_connection=True, n_classes=5, input_size_s=30, apply_softmax=False)
    ctx, dev = model.ctx, model.device
    cw = torch.tensor([1.0, 2.5, 0.7, 1.3, 1.9])
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    params = [k for k, e in model.entries.items() if e[0] == 0]
    for k in params:
        sd[k].requires_grad_(True)

    def timed(fn):
        ctx.timer_start(); fn(); return ctx.timer_stop_ms()

    def measure(variants):
        for fn in variants.values():
            for _ in range(3):
                fn()
        rounds = {k: [] for k in variants}; every = {k: [] for k in variants}
        for _ in range(args.rounds):
            ts = {k: [] for k in variants}
            for _ in range(args.iters):
                for k, fn in variants.items():
                    ts[k].append(timed(fn))
            for k in variants:
                rounds[k].append(sorted(ts[k])[len(ts[k]) // 2]); every[k] += ts[k]
        return {k: dict(median_ms=round(sorted(every[k])[len(every[k]) // 2], 4), round_medians_ms=[round(min(rounds[k]), 4), round(max(rounds[k]), 4)],
                        min_ms=round(min(every[k]), 4), max_ms=round(max(every[k]), 4)) for k in variants}

    for shape in args.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(B)
        x = torch.randn(B, 2, T, generator=g).to(dev)
        labels = torch.randint(0, 5, (B,), generator=g).to(dev)
        loss = torch.zeros(1, device=dev)
        cwd = cw.to(dev)

        def native_step():
            model.zero_grad()
            model.train_step(x, labels, class_weight=cwd, loss_out=loss)

        def native_forward():
            model.train()
            model.forward(x)

        def torch_step():
            for k in params:
                sd[k].grad = None
            y, _d, _b = usleep_forward(sd, x, depth=12, input_size=3000, training=True)
            F.cross_entropy(y, labels, weight=cwd, ignore_index=-1).backward()

        res = measure({"native_step": native_step, "native_forward": native_forward, "torch_step": torch_step})
        native_step()
        print(json.dumps(dict(what="usleep_train_step", B=B, T=T, iters=args.iters, rounds=args.rounds, native_step_launches=model.last_launches(), **res)), flush=True)


if __name__ == "__main__":
    main()
