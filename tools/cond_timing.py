"""Cost of class conditioning on the config_ldm UNet (bf16), one JSON line per measurement:

  * LDM train step at B = 256 (L = 768): unconditional vs conditional (num_classes 6, p_uncond 0.1) -- alternated, median of N
  * DDIM-50 at B = 256: conditional without guidance vs guidance_scale 3 (the forward runs 2B rows)
  * DDIM-50 at B = 1 with and without guidance (the few-row kernels; see `rocprofv3 --kernel-trace --stats` for which ran)

    python tools/cond_timing.py [--steps 10] [--only ddim_b1_guided]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", default=None, choices=[None, "train", "ddim_b256", "ddim_b1", "ddim_b1_guided"])
    args = ap.parse_args()
    import torch
    from eegldm.models import UNetModel
    from eegldm.schedulers import DDPMScheduler
    from eegldm.sampling import ddim_sample, make_sampling_scheduler
    from eegldm.training import ldm_train_step, randint, randn
    from make_golden_cases import UNET_FULL
    cfg = UNET_FULL[0]
    torch.manual_seed(0)
    plain = UNetModel(**cfg, dtype="bfloat16")
    cond = UNetModel(**dict(cfg, num_classes=6), dtype="bfloat16")
    sd = plain.state_dict()
    g = torch.Generator().manual_seed(42)
    sd = {k: (torch.randn(v.shape, generator=g) * 0.02 if float(v.abs().sum()) == 0.0 else v) for k, v in sd.items()}
    plain.load_state_dict(sd)
    cond.load_state_dict(dict(sd, **{"label_emb.weight": torch.randn(6, 512, generator=g)}))
    ctx, dev = plain.ctx, plain.device
    sched = DDPMScheduler(num_train_timesteps=1000, schedule="linear_beta", beta_start=0.0015, beta_end=0.0195, device=0)

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    if args.only in (None, "train"):
        B, L = 256, 768
        lat = randn(ctx, (B, 1, L), seed=1); nz = randn(ctx, (B, 1, L), seed=2)
        lab = randint(ctx, B, 5, seed=4)
        loss = torch.zeros(1, device=dev)

        def step(net, i):
            t = randint(ctx, B, 1000, seed=3, offset=i * B)
            net.zero_grad()
            kw = dict(labels=lab, p_uncond=0.1, null_class=5, seed=9, offset=i * B) if net is cond else {}
            ldm_train_step(net, sched, lat, nz, t, loss_out=loss, **kw)
        for net in (plain, cond):
            for i in range(3):
                step(net, i)
        times = {"plain": [], "cond": []}
        for i in range(args.steps):
            for name, net in (("plain", plain), ("cond", cond)):        # alternated: same host / clock conditions for both
                torch.cuda.synchronize(); t0 = time.perf_counter()
                step(net, i)
                torch.cuda.synchronize(); times[name].append(time.perf_counter() - t0)
        med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
        emit(what="ldm_train_step_b256_bf16", ms_uncond=round(med["plain"], 3), ms_cond=round(med["cond"], 3),
             ratio=round(med["cond"] / med["plain"], 4), spread_uncond_ms=[round(1e3 * min(times["plain"]), 3), round(1e3 * max(times["plain"]), 3)],
             spread_cond_ms=[round(1e3 * min(times["cond"]), 3), round(1e3 * max(times["cond"]), 3)], steps=args.steps)

    s50 = make_sampling_scheduler(50)

    def ddim(B, guided, reps):
        nz = randn(ctx, (B, 1, 768), seed=5)
        kw = dict(labels=[b % 5 for b in range(B)], guidance_scale=3.0 if guided else 1.0, null_class=5)
        ddim_sample(cond, None, s50, nz, crop=0, **kw)               # warm-up: table, arena, workspaces
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            ddim_sample(cond, None, s50, nz, crop=0, **kw)
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2]

    if args.only in (None, "ddim_b256"):
        a, b = ddim(256, False, 3), ddim(256, True, 3)
        emit(what="ddim50_b256_bf16_cond", s_no_guidance=round(a, 4), s_guidance3=round(b, 4), ratio=round(b / a, 3))
    if args.only in (None, "ddim_b1"):
        a, b = ddim(1, False, 5), ddim(1, True, 5)
        emit(what="ddim50_b1_bf16_cond", ms_no_guidance=round(1e3 * a, 2), ms_guidance3=round(1e3 * b, 2), ratio=round(b / a, 3))
    if args.only == "ddim_b1_guided":
        a = ddim(1, True, 2)
        emit(what="ddim50_b1_bf16_guided_profile_run", ms=round(1e3 * a, 2))


if __name__ == "__main__":
    main()
