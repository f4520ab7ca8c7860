"""Time of the frozen stage-1 encode (eegldm_aekl_encode, AutoencoderKL [32, 32, 64], norm_num_groups = 1) at the production shape of the LDM
step, (B, L) = (256, 3072), measured with the library's own HIP-event brackets (eegldm_timer_start / eegldm_timer_stop_ms) on the context's
stream, on the fused path (csrc/enc_fused.hip) and on the layer-by-layer path (EEGLDM_AEKL_NO_FUSED_ENC=1).

    python tools/enc_fused_timing.py [--dtype bf16] [--iters 30] [--rounds 5] [--baseline PATH/libeegldm.so] [--out FILE]

Every round is a fresh child process that loads ONE library (EEGLDM_LIB), warms both paths up and reports the median of --iters encodes of
each; with --baseline (a build of another commit) the rounds alternate between that library and this tree's, baseline first.  What a
difference between the two has to exceed is the spread of the round medians of the SAME library, printed beside them.  No figure is a gate."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

CHANNELS, B, L = [32, 32, 64], 256, 3072


def child(args):
    import torch
    from eegldm.models import AutoencoderKL
    ae = AutoencoderKL(spatial_dims=1, in_channels=1, out_channels=1, num_channels=CHANNELS, latent_channels=1, num_res_blocks=2,
                       norm_num_groups=1, attention_levels=[False] * len(CHANNELS), dtype={"bf16": "bfloat16", "f16": "float16"}[args.dtype])
    g = torch.Generator().manual_seed(0)
    sd = {}
    for k, v in ae.state_dict().items():
        if v.dim() == 1:
            sd[k] = (1.0 if k.endswith(".weight") else 0.0) + 0.1 * torch.randn(v.shape, generator=g)
        else:
            sd[k] = torch.randn(v.shape, generator=g) / (v.shape[1] * v.shape[2]) ** 0.5
    ae.load_state_dict(sd)
    x = torch.randn(args.batch, 1, args.length, generator=g).to(ae.device)
    out = {}
    for name, env in (("fused", None), ("layer_by_layer", "1")):
        if env is None:
            os.environ.pop("EEGLDM_AEKL_NO_FUSED_ENC", None)
        else:
            os.environ["EEGLDM_AEKL_NO_FUSED_ENC"] = env
        for _ in range(3):
            mu, _sg = ae.encode(x)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.iters):
            ae.ctx.timer_start()
            mu, _sg = ae.encode(x)
            ts.append(ae.ctx.timer_stop_ms())
        out[name] = sorted(ts)[len(ts) // 2]
        out[name + "_mu_abs_mean"] = float(mu.abs().mean())
    os.environ.pop("EEGLDM_AEKL_NO_FUSED_ENC", None)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=B)
    ap.add_argument("--length", type=int, default=L)
    ap.add_argument("--baseline", default=None, help="libeegldm.so of the commit to compare with")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    libs = ([("baseline", args.baseline)] if args.baseline else []) + [("this tree", None)]
    res = {n: {"fused": [], "layer_by_layer": []} for n, _ in libs}
    lines = []
    for r in range(args.rounds):
        for name, path in libs:
            env = dict(os.environ)
            if path:
                env["EEGLDM_LIB"] = os.path.abspath(path)
            else:
                env.pop("EEGLDM_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--dtype", args.dtype, "--iters", str(args.iters), "--batch", str(args.batch),
                   "--length", str(args.length)]
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
            if p.returncode != 0:
                print(p.stdout[-2000:])
                raise SystemExit(f"round {r} ({name}) ended with status {p.returncode}: nothing further is started")
            rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            for k in ("fused", "layer_by_layer"):
                res[name][k].append(rec[k])
            line = json.dumps(dict(round=r, library=name, **rec))
            print(line, flush=True); lines.append(line)
    for name, _ in libs:
        for k, v in res[name].items():
            s = sorted(v)
            line = (f"{name:>9s} {k:>14s}: median of {len(v)} round medians {1e3 * s[len(s) // 2]:8.1f} us, rounds {1e3 * s[0]:.1f} .. {1e3 * s[-1]:.1f} us "
                    f"(spread {100 * (s[-1] - s[0]) / s[len(s) // 2]:.1f} %)   [{args.dtype}, B {args.batch}, L {args.length}, {args.iters} encodes per round]")
            print(line); lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
