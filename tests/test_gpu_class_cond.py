"""-m gpu: class-conditional UNet (num_classes, unet.py:342,366,379-380,531-533) and classifier-free guided sampling.

Goldens: tests/golden/unet_cond_*.npz, produced by the imported reference (tests/golden/make_golden_cond.py).  16-bit storage is bounded by
the storage gap of the test-local restatement (tests/cond_unet.py) run with oracle.quant's emulated storage."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from make_golden_cond import COND_CASES, golden_path  # noqa: E402
from param_gen import gen_param, normal, timesteps  # noqa: E402


def _sd(net, seed):
    return {k: torch.from_numpy(gen_param(seed, k, shape)) for k, (_o, _n, shape) in net.entries.items()}


def _net(name, dtype="float32"):
    from eegldm.models import UNetModel
    kw, B, L, labels, seed = COND_CASES[name]
    net = UNetModel(**kw, dtype=dtype)
    sd = _sd(net, seed)
    net.load_state_dict(sd)
    return net, sd, kw, B, L, labels, seed


def _digest_check(grads, g, keys):
    gscale = max(float(g["g_l2:" + k]) for k in keys)
    for k in keys:
        gr = grads[k].double().reshape(-1).cpu(); l2 = float(g["g_l2:" + k]); floor = 1e-3 * gscale
        rel = abs(float(gr.norm()) - l2) / (l2 + floor)
        head = g["g_head:" + k].astype(np.float64)
        he = float(np.linalg.norm(gr[:16].numpy() - head[:16])) / (float(np.linalg.norm(head[:16])) + floor / np.sqrt(max(1, gr.numel() / 16)))
        se = abs(float(gr.sum()) - float(g["g_sum:" + k])) / (abs(float(g["g_sum:" + k])) + l2 + floor)
        assert rel < 1e-3 and he < 2e-3 and se < 2e-3, f"{k}: norm {rel:.2e} head {he:.2e} sum {se:.2e}"


@pytest.mark.parametrize("name", ["small_k5", "full_k6"])
def test_conditional_unet_fp32_vs_reference_golden(name):
    import gpu_util as G
    net, sd, kw, B, L, labels, seed = _net(name)
    g = np.load(golden_path(name))
    assert list(net.entries) == [str(k) for k in g["keys"]] and len(net.entries) == 279
    x = torch.from_numpy(normal((B, kw["in_channels"], L), seed=seed + 1)); t = torch.from_numpy(g["t"])
    y = net(x, timesteps=t, y=torch.tensor(labels))
    net.zero_grad()
    dx = net.backward(torch.from_numpy(normal(tuple(y.shape), seed=seed + 3)), need_dx=True)
    G.assert_close(y, g["y"], rtol=2e-4, atol=5e-5, name="y")
    G.assert_close(dx, g["dx"], rtol=2e-3, atol=5e-5, name="dx")
    grads = net.grad_dict()
    _digest_check(grads, g, net.entries)
    ge = grads["label_emb.weight"].cpu()
    G.assert_close(ge, g["g_label_emb"], rtol=2e-3, atol=1e-5 * float(np.abs(g["g_label_emb"]).max()), name="label_emb grad")
    absent = [c for c in range(kw["num_classes"]) if c not in labels]
    assert absent and torch.count_nonzero(ge[absent]) == 0       # classes absent from the batch: exactly zero


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_conditional_unet_16bit_within_storage_gap(dtype):
    import gpu_util as G
    from cond_unet import unet_forward_cond
    from oracle import quant as Q
    net, sd, kw, B, L, labels, seed = _net("small_k5", dtype)
    x = torch.from_numpy(normal((B, kw["in_channels"], L), seed=seed + 1)); t = torch.from_numpy(timesteps(B, seed=seed + 2))
    dy = torch.from_numpy(normal((B, kw["out_channels"], L), seed=seed + 3)); lab = torch.tensor(labels)
    y = net(x, timesteps=t, y=lab)
    net.zero_grad()
    dx = net.backward(dy, need_dx=True)

    def run(emul):
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        xr = x.clone().requires_grad_(True)
        with Q.bf16_storage(emul, torch.bfloat16 if dtype == "bfloat16" else torch.float16):
            yo = unet_forward_cond(p, kw, xr, t, lab)
            yo.backward(dy)
        return yo.detach(), xr.grad, {k: v.grad for k, v in p.items()}
    y32, dx32, g32 = run(False)
    yq, dxq, gq = run(True)
    floor = G.BF16_FLOOR if dtype == "bfloat16" else G.F16_FLOOR
    assert G.rel_l2(y, y32) < G.bf16_gap_bound(G.rel_l2(yq, y32), floor=floor)
    assert G.rel_l2(dx, dx32) < G.bf16_gap_bound(G.rel_l2(dxq, dx32), floor=floor)
    print(G.assert_bf16_grads(net.grad_dict(), g32, gq, f"conditional UNet {dtype}", floor=floor))


def test_key_order_and_reference_state_dict_roundtrip():
    from eegldm.models import UNetModel
    kw = COND_CASES["full_k6"][0]
    g = np.load(golden_path("full_k6"))
    net = UNetModel(**kw)
    assert list(net.state_dict()) == [str(k) for k in g["keys"]] and net.entries["label_emb.weight"][2] == (6, 512)
    sd = _sd(net, 5)
    net.load_state_dict({"module." + k: v for k, v in sd.items()})         # DataParallel prefix
    assert torch.equal(net.state_dict()["label_emb.weight"].cpu(), sd["label_emb.weight"])
    # the label row lies outside the slice the grad hook reports early
    off, n, _s = net.entries["label_emb.weight"]
    assert off + n <= net.entries["middle_block.0.in_layers.0.weight"][0]
    # nn.Embedding's default init: N(0, 1), not the fan-in bound
    net.reset_parameters(torch.Generator().manual_seed(0))
    w = net.state_dict()["label_emb.weight"]
    assert 0.9 < float(w.std()) < 1.1


def test_train_step_equals_composition_and_autograd_bridge():
    from eegldm.schedulers import DDPMScheduler
    from eegldm.training import ldm_train_step
    net, sd, kw, B, L, labels, seed = _net("small_k5")
    sched = DDPMScheduler(num_train_timesteps=1000, schedule="linear_beta", beta_start=0.0015, beta_end=0.0195)
    dev = net.device
    lat = torch.from_numpy(normal((B, 1, L), seed=11)).to(dev); nz = torch.from_numpy(normal((B, 1, L), seed=12)).to(dev)
    t = torch.from_numpy(timesteps(B, seed=13)).to(dev); lab = torch.tensor(labels, device=dev)
    net.train(); net.zero_grad()
    loss = ldm_train_step(net, sched, lat, nz, t, labels=lab)
    g_native = net.flat_grad.clone()
    # composition through the conditional forward entry
    net.zero_grad()
    with torch.no_grad():
        noisy = sched.add_noise(original_samples=lat, noise=nz, timesteps=t)
        pred = net(noisy, timesteps=t, y=lab)
        d = 2.0 * (pred - nz) / pred.numel()
        net.backward(d)
    g_comp = net.flat_grad.clone()
    assert abs(float(loss) - float(((pred - nz) ** 2).mean())) <= 1e-5 * float(loss)
    assert float((g_native - g_comp).norm() / g_comp.norm()) < 1e-5
    assert float(g_native[net.entries["label_emb.weight"][0]:][:5 * 512].abs().sum()) > 0
    # autograd bridge: parameters() under a torch loss, with a second forward (other labels) before the backward
    p = net.parameters()[0]
    p.grad = None
    out = net(noisy, timesteps=t, y=lab)
    _other = net(noisy, timesteps=t, y=torch.zeros_like(lab))           # rewrites the executor's tape
    torch.nn.functional.mse_loss(out, nz).backward()
    assert float((p.grad - g_comp).norm() / g_comp.norm()) < 1e-5


def test_label_dropout_statistics_and_reproducibility():
    from eegldm.training import label_dropout
    import eegldm
    ctx = eegldm.default_context(0)
    n, p = 200000, 0.1
    y = torch.randint(0, 5, (n,), device="cuda")
    a = label_dropout(ctx, y, p, 5, seed=7, offset=3)
    b = label_dropout(ctx, y, p, 5, seed=7, offset=3)
    assert torch.equal(a, b)
    repl = int((a == 5).sum())
    sd = (n * p * (1 - p)) ** 0.5
    assert abs(repl - n * p) < 5 * sd, (repl, n * p)
    assert torch.equal(a[a != 5], y[a != 5])
    assert torch.equal(label_dropout(ctx, y, 0.0, 5, seed=7, offset=3), y)
    assert not torch.equal(label_dropout(ctx, y, p, 5, seed=8, offset=3), a)


def _grads_of_step(net, sched, lat, nz, t, lab, **kw):
    from eegldm.training import ldm_train_step
    net.zero_grad()
    ldm_train_step(net, sched, lat, nz, t, labels=lab, **kw)
    return net.flat_grad.clone()


def test_train_step_label_dropout_semantics_and_determinism():
    from eegldm._lib import set_deterministic
    from eegldm.schedulers import DDPMScheduler
    from eegldm.training import Adam
    net, sd, kw, B, L, labels, seed = _net("small_k5")
    sched = DDPMScheduler(num_train_timesteps=1000, schedule="linear_beta", beta_start=0.0015, beta_end=0.0195)
    dev = net.device
    lat = torch.from_numpy(normal((B, 1, L), seed=21)).to(dev); nz = torch.from_numpy(normal((B, 1, L), seed=22)).to(dev)
    t = torch.from_numpy(timesteps(B, seed=23)).to(dev); lab = torch.tensor(labels, device=dev)
    net.train()
    set_deterministic(True)
    try:
        g0 = _grads_of_step(net, sched, lat, nz, t, lab)
        assert torch.equal(_grads_of_step(net, sched, lat, nz, t, lab, p_uncond=0.0, null_class=4, seed=99), g0)   # p = 0: no dropout
        g1 = _grads_of_step(net, sched, lat, nz, t, lab, p_uncond=1.0, null_class=2, seed=5)
        assert torch.equal(g1, _grads_of_step(net, sched, lat, nz, t, torch.full_like(lab, 2)))                 # p = 1: all null
        # N conditional steps with dropout, twice from the same state: bit-identical
        def run():
            net.load_state_dict(sd); opt = Adam(net, lr=1e-3)
            for i in range(3):
                _grads_of_step(net, sched, lat, nz, t, lab, p_uncond=0.5, null_class=4, seed=11, offset=i * B)
                opt.step()
            return net.flat.clone()
        assert torch.equal(run(), run())
    finally:
        set_deterministic(False)


def _tiny_cond(seed=71, K=3):
    from eegldm.models import UNetModel
    from make_golden_cases import UNET_CASES
    kw = dict(UNET_CASES["tiny_l64"][0], num_classes=K)
    net = UNetModel(**kw)
    sd = _sd(net, seed)
    net.load_state_dict(sd)
    return net, sd, kw


@pytest.mark.parametrize("graph", [False, True])
def test_conditional_sampler_matches_hostloop(graph):
    import gpu_util as G
    from eegldm.sampling import ddim_sample, ddim_sample_hostloop, make_sampling_scheduler
    net, sd, kw = _tiny_cond()
    B, L, steps = 5, 64, 8
    noise = torch.from_numpy(normal((B, 1, L), seed=72))
    lab = [2, 0, 1, 2, 0]
    sched = make_sampling_scheduler(steps)
    info = {}
    _w, z = ddim_sample(net, None, sched, noise, crop=0, use_graph=graph, info=info, labels=lab)
    assert info["graph"] == graph
    _w, zh = ddim_sample_hostloop(net, None, sched, noise, crop=0, labels=lab)
    assert G.rel_l2(z, zh) < 2e-5, G.rel_l2(z, zh)
    # a mixed-label batch == per-class sub-batches
    for c in range(3):
        idx = [i for i, v in enumerate(lab) if v == c]
        _w, zc = ddim_sample(net, None, sched, noise[idx], crop=0, use_graph=graph, labels=c)
        assert G.rel_l2(z[idx], zc) < 2e-5
    # guidance_scale = 1 is the plain conditional sampler, bit for bit
    _w, z1 = ddim_sample(net, None, sched, noise, crop=0, use_graph=graph, labels=lab, guidance_scale=1.0, null_class=1)
    assert torch.equal(z1, z)
    # guidance 3 == the host loop that calls the UNet on cond and null labels and mixes the outputs
    _w, zg = ddim_sample(net, None, sched, noise, crop=0, use_graph=graph, labels=lab, guidance_scale=3.0, null_class=1)
    _w, zgh = ddim_sample_hostloop(net, None, sched, noise, crop=0, labels=lab, guidance_scale=3.0, null_class=1)
    assert G.rel_l2(zg, zgh) < 5e-5, G.rel_l2(zg, zgh)
    assert G.rel_l2(zg, z) > 1e-3
    # again (cached state / graph replay): identical
    _w, zg2 = ddim_sample(net, None, sched, noise, crop=0, use_graph=graph, labels=lab, guidance_scale=3.0, null_class=1)
    assert torch.equal(zg2, zg)


@pytest.mark.parametrize("guidance", [1.0, 2.5])
def test_conditional_ancestral_sampler_vs_loop(guidance):
    """DDPM (ancestral) steps: the on-device Philox noise is reproduced through eegldm_randn and fed to a host loop."""
    import gpu_util as G
    from eegldm.schedulers import DDPMScheduler
    from eegldm.sampling import ddim_sample
    from eegldm.training import randn
    net, sd, kw = _tiny_cond(81)
    B, L, seed = 3, 64, 5
    nz0 = torch.from_numpy(normal((B, 1, L), seed=82)).to(net.device)
    lab = torch.tensor([1, 1, 0], device=net.device)
    sched = DDPMScheduler(num_train_timesteps=1000, schedule="linear_beta", beta_start=0.0015, beta_end=0.0195, clip_sample=True)
    sched.timesteps = torch.tensor([400, 300, 2, 1, 0])
    for graph in (False, True):
        _w, lat = ddim_sample(net, None, sched, nz0, crop=0, seed=seed, use_graph=graph, labels=lab.tolist(), guidance_scale=guidance, null_class=2)
        x, n = nz0.clone(), B * L
        net.eval()
        with torch.no_grad():
            for i, tt in enumerate([400, 300, 2, 1, 0]):
                tv = torch.full((B,), tt, device=net.device)
                out = net(x, timesteps=tv, y=lab)
                if guidance != 1.0:
                    ou = net(x, timesteps=tv, y=torch.full_like(lab, 2))
                    out = ou + guidance * (out - ou)
                eps = randn(net.ctx, (B, 1, L), seed=seed, offset=i * ((n + 3) // 4))
                x, _ = sched.step(out, tt, x, noise=eps)
        assert G.rel_l2(lat, x) < 1e-4, (graph, G.rel_l2(lat, x))


def test_sampler_batch_sizes_and_row_counts():
    """B = 1 and B = 256 run; with guidance a B = 1 run is a 2-row forward (the sampler state is keyed by the forward's rows)."""
    from eegldm.sampling import ddim_sample, make_sampling_scheduler
    net, sd, kw = _tiny_cond(91)
    sched = make_sampling_scheduler(4)
    for B in (1, 256):
        noise = torch.from_numpy(normal((B, 1, 64), seed=92))
        _w, z = ddim_sample(net, None, sched, noise, crop=0, labels=[b % 3 for b in range(B)], guidance_scale=2.0, null_class=0)
        assert z.shape == (B, 1, 64) and torch.isfinite(z).all()
        _w, z1 = ddim_sample(net, None, sched, noise, crop=0, labels=1)
        assert torch.isfinite(z1).all()
    # B = 1 with guidance and B = 2 without share one (2-row) sampler state: both still right
    n1 = torch.from_numpy(normal((1, 1, 64), seed=93)); n2 = torch.from_numpy(normal((2, 1, 64), seed=94))
    a = ddim_sample(net, None, sched, n1, crop=0, labels=[2], guidance_scale=2.0, null_class=0)[1]
    b = ddim_sample(net, None, sched, n2, crop=0, labels=[2, 1])[1]
    assert torch.equal(ddim_sample(net, None, sched, n1, crop=0, labels=[2], guidance_scale=2.0, null_class=0)[1], a)
    assert torch.equal(ddim_sample(net, None, sched, n2, crop=0, labels=[2, 1])[1], b)


def test_errors():
    from eegldm._lib import lib
    from eegldm.models import UNetModel
    from eegldm.sampling import ddim_sample, make_sampling_scheduler
    from eegldm.schedulers import DDPMScheduler
    from eegldm.training import ldm_train_step
    from make_golden_cases import UNET_CASES
    net, sd, kw = _tiny_cond(95)
    x = torch.zeros(2, 1, 64); t = torch.tensor([1, 2])
    with pytest.raises(IndexError):
        net(x, timesteps=t, y=torch.tensor([0, 3]))
    with pytest.raises(IndexError):
        net(x, timesteps=t, y=torch.tensor([-1, 0]))
    with pytest.raises(AssertionError, match="must specify y if and only if the model is class-conditional"):
        net(x, timesteps=t)
    with pytest.raises(AssertionError):
        net(x, timesteps=t, y=torch.tensor([0, 1, 2]))
    with pytest.raises(IndexError):
        ddim_sample(net, None, make_sampling_scheduler(2), x, crop=0, labels=[0, 5])
    # the unconditional entry points refuse a conditional UNet (no silent class 0)
    out = torch.empty_like(x).cuda(); xc = x.cuda(); tc = t.cuda()
    assert lib.eegldm_unet_forward(net.h, xc.data_ptr(), tc.data_ptr(), out.data_ptr(), 2, 64, 0) != 0
    assert b"class-conditional" in lib.eegldm_last_error()
    sched = DDPMScheduler(num_train_timesteps=1000, schedule="linear_beta", beta_start=0.0015, beta_end=0.0195)
    loss = torch.zeros(1, device="cuda")
    assert lib.eegldm_ldm_train_step(net.h, xc.data_ptr(), xc.data_ptr(), tc.data_ptr(), sched._acp_dev.data_ptr(), 0, 2, 64, 1.0,
                                     loss.data_ptr()) != 0
    with pytest.raises(ValueError):
        ldm_train_step(net, sched, xc, xc, tc)
    # and the conditional ones refuse an unconditional UNet; y on an unconditional model is still ignored
    plain = UNetModel(**UNET_CASES["tiny_l64"][0]); plain.eval()
    lab = torch.tensor([0, 1], device="cuda")
    assert lib.eegldm_unet_forward_cond(plain.h, xc.data_ptr(), tc.data_ptr(), lab.data_ptr(), out.data_ptr(), 2, 64, 0) != 0
    assert torch.equal(plain(x, timesteps=t, y=lab), plain(x, timesteps=t))
    with pytest.raises(NotImplementedError):
        UNetModel(**dict(UNET_CASES["tiny_l64"][0], num_classes=3, n_embed=16))


def test_entry_scripts_conditional_train_and_guided_sample(tmp_path):
    """train_ldm with num_classes from the yaml, stage files beside the recordings and label dropout; then sample_trials with a labels
    file and guidance, labels recorded beside the windows."""
    import yaml
    from eegldm.entry import train_ldm as TL, sample_trials as ST
    from eegldm.models import AutoencoderKL
    from test_gpu_entry import AEKL_YAML, LDM_YAML
    out = str(tmp_path)
    rec = tmp_path / "rec"; rec.mkdir()
    r = np.random.default_rng(0)
    for i in range(4):
        np.save(rec / f"night{i}.npy", (1e-5 * r.standard_normal((1, 15000))).astype(np.float64))
        np.save(rec / f"night{i}.stages.npy", np.array([0, 2, -1, 4, 3], np.int64))
    a_yaml, l_yaml = os.path.join(out, "aekl.yaml"), os.path.join(out, "ldm.yaml")
    a = dict(AEKL_YAML); a["train"] = dict(a["train"], output_dir=out)
    l = {"train": dict(LDM_YAML["train"], output_dir=out), "model": {"params": dict(LDM_YAML["model"]["params"])}}
    l["model"]["params"]["unet_config"] = {"params": dict(LDM_YAML["model"]["params"]["unet_config"]["params"], num_classes=6)}
    yaml.safe_dump(a, open(a_yaml, "w")); yaml.safe_dump(l, open(l_yaml, "w"))
    ae = AutoencoderKL(**a["autoencoderkl"]["params"])
    run_a = os.path.join(out, "aekl"); os.makedirs(run_a)
    torch.save({k: v.cpu() for k, v in ae.state_dict().items()}, os.path.join(run_a, "best_model.pth"))
    run_l = TL.main(TL.parse_args(["--config_file", l_yaml, "--autoencoderkl_config_file_path", a_yaml, "--best_model_path", run_a,
                                   "--path_pre_processed", str(rec), "--latent_channels", "1", "--max_steps", "2", "--p_uncond", "0.2"]))
    ck = torch.load(os.path.join(run_l, "checkpoint.pth"))
    assert tuple(ck["diffusion"]["label_emb.weight"].shape) == (6, 128) and list(ck["diffusion"])[4] == "label_emb.weight"
    assert float(ck["diffusion"]["label_emb.weight"].abs().sum()) > 0
    lab_file = os.path.join(out, "labels.txt"); np.savetxt(lab_file, np.array([4, 0, 2]), fmt="%d")
    sdir = ST.main(ST.parse_args(["--output_dir", out, "--best_model_path", run_a, "--diffusion_path", run_l,
                                  "--autoencoderkl_config_file_path", a_yaml, "--ldm_config_file_path", l_yaml, "--start_seed", "3",
                                  "--stop_seed", "6", "--num_inference_steps", "4", "--latent_channels", "1", "--labels_file", lab_file,
                                  "--guidance_scale", "3", "--null_class", "5"]))
    for i, c in zip((3, 4, 5), (4, 0, 2)):
        s = np.load(os.path.join(sdir, f"sample_{i}.npy"))
        assert s.shape == (1, 1, 3000) and np.isfinite(s).all()
        assert np.load(os.path.join(sdir, f"sample_{i}_label.npy")).tolist() == [c]
