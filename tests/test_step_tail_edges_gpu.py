"""The training step's tail kernels (csrc/model_kernels.hip) at the grid, chunk and cluster-count edges that the
default-shape tests in test_model_gpu.py do not reach: gradient norm, clip + AdamW, BatchNorm / LayerNorm + LeakyReLU,
the latent head and the K-means / OT cluster losses, each against an fp64 reference.

The cases, the branch each one is there for and the references are in step_tail_cases.py; test_step_tail_ref_cpu.py
checks on the CPU that every case reaches its branch.  These are the smallest shapes that enter each branch."""
import numpy as np
import pytest
import torch

import step_tail_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spadot_amd import ops
    return ops


def f32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()


def i64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int64, device=DEV).contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def worst_ratio(a, r, rtol, atol):
    """max |a - r| / (atol + rtol |r|): at most 1 where assert_allclose(a, r, rtol, atol) holds."""
    a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return float((np.abs(a - r) / (atol + rtol * np.abs(r))).max())


# ------------------------------------------------------------------ gradient norm: the two entries, called directly

@pytest.mark.parametrize("case", C.SUMSQ_CASES, ids=lambda c: str(c["count"]))
def test_grad_norm_entries_at_tail_and_grid_edges(ops, case):
    """spadot_grad_sumsq and spadot_grad_norm_step_dev on counts that FlatAdamW (which pads to 4) never passes: the scalar
    tail alone, the tail beside one workgroup, the first live float4 of unroll lane u = 1, a second trip of the k loop
    with 2048 partials for the 1024-thread final sum.  fp64 accumulation, one rounding to fp32; reproducible bits; the
    step count advances by exactly one per call of the _step_dev entry."""
    count = case["count"]
    g = C.sumsq_values(count)
    ref = C.sumsq_ref(g)
    gd = torch.from_numpy(g).to(DEV)
    assert gd.data_ptr() % 16 == 0
    lib = ops.model_lib()
    scratch = torch.empty(4096, dtype=torch.float64, device=DEV)
    out = torch.empty(1, dtype=torch.float32, device=DEV)
    step = torch.tensor([41], dtype=torch.int32, device=DEV)
    got = {"sumsq": [], "norm_step": []}
    for call in range(2):
        scratch.fill_(float("nan")); out.fill_(-1.0)              # a partial that is read but was not written shows
        assert lib.spadot_grad_sumsq(gd.data_ptr(), count, scratch.data_ptr(), out.data_ptr(), _stream()) == 0
        got["sumsq"].append(out.clone())
        scratch.fill_(float("nan")); out.fill_(-1.0)
        assert lib.spadot_grad_norm_step_dev(gd.data_ptr(), count, scratch.data_ptr(), out.data_ptr(), step.data_ptr(), _stream()) == 0
        got["norm_step"].append(out.clone())
        assert int(step.item()) == 41 + call + 1
    for name, (first, second) in got.items():
        err = abs(float(first.item()) - ref) / ref
        print(f"{name}: count {count} got {float(first.item())!r} ref {ref!r} rel err {err:.3e} (bound {C.SUMSQ_RTOL:.3e})")
        assert torch.equal(first, second), name
        assert abs(float(first.item()) - ref) <= C.SUMSQ_RTOL * ref, (name, float(first.item()), ref)


# ------------------------------------------------------------------ clip + AdamW through FlatAdamW

@pytest.fixture(scope="module")
def adamw_run(ops):
    """Three optimizers over clones of the same 8.4 M parameters -- (a) step() without images, (b) step() with bf16 images,
    (c) step_head() + step_rest() with the same images and `first` / `last` groups -- stepped three times (clipped,
    unclipped, grad_scale 0.25 on gradients 4x as large) from step count 20 000, beside the fp64 reference.  Returns, per
    step, what the tests assert: equalities (computed on the device) and the worst error ratios against the reference."""
    case = C.ADAMW_CASE
    base = C.adamw_params(case)
    hyper = dict(lr=case["lr"], betas=case["betas"], eps=case["eps"], weight_decay=case["wd"], max_norm=case["max_norm"])

    def make(images, first=(), last=()):
        ps = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in base]
        opt = ops.FlatAdamW(ps, first=[ps[i] for i in first] or None, last=[ps[i] for i in last] or None, **hyper)
        imgs = {}
        if images:
            for i, Kp in case["images"].items():
                imgs[i] = torch.full((case["shapes"][i][0], Kp), 5.0, dtype=torch.bfloat16, device=DEV)
                assert opt.maintain_image(ps[i], imgs[i])
        opt.step_dev.fill_(case["step0"])
        return ps, opt, imgs

    pa, oa, _ = make(False)
    pb, ob, ib = make(True)
    pc, oc, ic = make(True, case["first"], case["last"])
    assert oa.count == ob.count == oc.count == case["padded"]
    assert oc.head_count == case["head_count"] and oc.params[0] is pc[case["first"][0]] and oc.params[-1] is pc[case["last"][0]]

    def moments(opt, p):
        off = (p.data_ptr() - opt.flat_param.data_ptr()) // 4
        return opt.exp_avg[off:off + p.numel()], opt.exp_avg_sq[off:off + p.numel()]

    rp = [a.astype(np.float64) for a in base]
    rm, rv = [np.zeros_like(a) for a in rp], [np.zeros_like(a) for a in rp]
    steps = []
    for s, st in enumerate(case["steps"]):
        grads = C.adamw_grads(case, s)
        gdev = [torch.from_numpy(g).to(DEV) for g in grads]
        for ps, opt in ((pa, oa), (pb, ob), (pc, oc)):
            for p, g in zip(ps, gdev):
                p.grad.copy_(g)
            opt.grad_scale.fill_(st["grad_scale"])
        oa.step()
        ob.step()
        oc.step_head(); oc.step_rest()
        torch.cuda.synchronize()
        rp, rm, rv, rsumsq = C.clip_adamw_ref(rp, grads, rm, rv, case["step0"] + s + 1, case["lr"], case["betas"], case["eps"],
                                              case["wd"], case["max_norm"], st["grad_scale"])
        rec = {"step_dev": [int(o.step_dev.item()) for o in (oa, ob, oc)], "sumsq": [float(o.sumsq.item()) for o in (oa, ob, oc)],
               "sumsq_equal": torch.equal(oa.sumsq, ob.sumsq) and torch.equal(oa.sumsq, oc.sumsq), "ref_sumsq": rsumsq,
               "identical": [], "images": [], "pads": [], "ratio": {"p": 0.0, "m": 0.0, "v": 0.0}}
        for i in range(len(base)):
            ma, va = moments(oa, pa[i])
            for ps, opt in ((pb, ob), (pc, oc)):
                mx, vx = moments(opt, ps[i])
                rec["identical"].append(torch.equal(pa[i].detach(), ps[i].detach()) and torch.equal(ma, mx) and torch.equal(va, vx))
            rec["ratio"]["p"] = max(rec["ratio"]["p"], worst_ratio(pa[i].detach().cpu().numpy(), rp[i], case["rtol"], case["atol"]))
            for key, dev_t, r, rtol in (("m", ma, rm[i], case["m_rtol"]), ("v", va, rv[i], case["v_rtol"])):
                r = r.reshape(-1)
                rec["ratio"][key] = max(rec["ratio"][key], worst_ratio(dev_t.cpu().numpy(), r, rtol, rtol * np.abs(r).max()))
        for ps, imgs in ((pb, ib), (pc, ic)):
            for i, im in imgs.items():
                K = case["shapes"][i][1]
                rec["images"].append(torch.equal(im[:, :K], ps[i].detach().bfloat16()))
                rec["pads"].append(bool((im[:, K:] == 5.0).all()))
        rec["images_equal"] = all(torch.equal(ib[i], ic[i]) for i in ib)
        steps.append(rec)
    return steps


def test_clip_adamw_three_forms_are_bit_identical_past_the_grid(adamw_run):
    """step() without images (k_adamw, grid-strided), step() with images (k_adamw_img, grid-strided) and step_head() +
    step_rest() (the range entry, 512 workgroups, image offsets relative to a base > 0) leave the same bits in the
    parameters, both moments, the squared norm and the step count, after each of the three steps."""
    for s, rec in enumerate(adamw_run):
        assert rec["step_dev"] == [C.ADAMW_CASE["step0"] + s + 1] * 3, (s, rec["step_dev"])
        assert rec["sumsq_equal"], (s, rec["sumsq"])
        assert all(rec["identical"]), (s, rec["identical"])


def test_clip_adamw_images_follow_the_parameters_and_pads_stay(adamw_run):
    for s, rec in enumerate(adamw_run):
        assert len(rec["images"]) == 4 and all(rec["images"]), (s, rec["images"])      # image == param.bfloat16(), bitwise
        assert all(rec["pads"]), (s, rec["pads"])                                      # columns K.. of the padded image untouched
        assert rec["images_equal"], s


def test_clip_adamw_matches_fp64_reference_past_the_grid(adamw_run):
    """Parameters, both moments and the squared norm against clip_adamw_ref after each step (clipped, unclipped,
    grad_scale = 0.25), with bias corrections of step 20 001 and up."""
    case = C.ADAMW_CASE
    for s, rec in enumerate(adamw_run):
        print(f"step {s}: sumsq {rec['sumsq'][0]!r} ref {rec['ref_sumsq']!r}; worst |err| / (atol + rtol |ref|): "
              f"p {rec['ratio']['p']:.3f} (rtol {case['rtol']:g} atol {case['atol']:g}), m {rec['ratio']['m']:.3f} "
              f"(rtol {case['m_rtol']:.3g}), v {rec['ratio']['v']:.3f} (rtol {case['v_rtol']:.3g})")
    for s, rec in enumerate(adamw_run):
        assert abs(rec["sumsq"][0] - rec["ref_sumsq"]) <= C.SUMSQ_RTOL * rec["ref_sumsq"], (s, rec["sumsq"][0], rec["ref_sumsq"])
        assert rec["ratio"]["p"] <= 1.0 and rec["ratio"]["m"] <= 1.0 and rec["ratio"]["v"] <= 1.0, (s, rec["ratio"])


# ------------------------------------------------------------------ BatchNorm / LayerNorm + LeakyReLU

@pytest.mark.parametrize("case", C.BN_CASES, ids=lambda c: f"{c['b']}-{c['F']}-{c['dtype']}-{'bias' if c['bias'] else 'nobias'}")
def test_bn_act_looped_path_and_edges(ops, case):
    """ops.bn_act past the 512-row register path (float and bf16 input, with and without the Linear bias), with two rows and
    with one feature: output, running statistics, counter and all gradients against nn.BatchNorm1d in fp64."""
    F_, dt = case["F"], getattr(torch, case["dtype"])
    x, lb, w, gamma, beta = C.bn_inputs(case)
    ref = C.bn_reference(case)
    bn = torch.nn.BatchNorm1d(F_).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(gamma.float()); bn.bias.copy_(beta.float())
    xd = x.to(DEV, dt).requires_grad_(True)
    lbd = None if lb is None else lb.to(DEV, torch.float32).requires_grad_(True)
    yd = ops.bn_act(xd, lbd, bn, 0.01)
    (yd * w.to(DEV, torch.float32)).sum().backward()
    tol = 2e-2 if dt == torch.bfloat16 else 2e-4
    np.testing.assert_allclose(yd.detach().cpu().numpy(), ref["y"].numpy(), rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), ref["running_mean"].numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), ref["running_var"].numpy(), rtol=1e-5, atol=1e-6)
    assert int(bn.num_batches_tracked) == ref["count"] == 1
    for name, a, r in (("x", xd.grad, ref["dx"]), ("gamma", bn.weight.grad, ref["dgamma"]), ("beta", bn.bias.grad, ref["dbeta"])):
        r = r.numpy()
        print(f"d{name}: worst |err| / (tol (|ref| + max |ref|)) = {worst_ratio(a.float().cpu().numpy(), r, tol, tol * np.abs(r).max()):.3f}")
        np.testing.assert_allclose(a.float().cpu().numpy(), r, rtol=tol, atol=tol * np.abs(r).max(), err_msg=name)
    if lbd is not None:
        assert float(lbd.grad.abs().max()) == 0.0                   # the batch mean removes the shift


@pytest.mark.parametrize("case", C.LN_CASES, ids=lambda c: f"{c['b']}-{c['F']}")
def test_ln_act_idle_lanes_ragged_columns_and_one_feature(ops, case):
    """ops.ln_act with F < 64 (idle lanes in the wave sums), F % 16 != 0 beside more than 64 rows (the column pass loops),
    b % 4 != 0 over several workgroups, and F = 1 (y = leaky(beta), dx = 0)."""
    b, F_ = case["b"], case["F"]
    x, w, gamma, beta = C.ln_inputs(case)
    ref = C.ln_reference(case)
    ln = torch.nn.LayerNorm(F_).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(gamma.float()); ln.bias.copy_(beta.float())
    xd = x.to(DEV, torch.float32).requires_grad_(True)
    yd = ops.ln_act(xd, ln, 0.01)
    (yd * w.to(DEV, torch.float32)).sum().backward()
    np.testing.assert_allclose(yd.detach().cpu().numpy(), ref["y"].numpy(), rtol=2e-4, atol=2e-5)
    grads = {"x": (xd.grad, ref["dx"]), "gamma": (ln.weight.grad, ref["dgamma"]), "beta": (ln.bias.grad, ref["dbeta"])}
    if F_ == 1:
        # one feature: x - mean is exactly 0, so y = leaky(beta) in every row and nothing flows to x or gamma (the fp64
        # reference leaves rounding dust of 1e-16 there: compared with 0, not with the dust)
        want = float(torch.nn.functional.leaky_relu(beta, 0.01))
        assert bool((yd.detach() == yd.detach()[0]).all()) and float(yd.detach()[0]) == pytest.approx(want, rel=2e-6)
        assert float(xd.grad.abs().max()) == 0.0 and float(ln.weight.grad.abs().max()) == 0.0
        assert float(ref["dx"].abs().max()) < 1e-12 and float(ref["dgamma"].abs().max()) < 1e-12
        grads = {"beta": grads["beta"]}
    for name, (a, r) in grads.items():
        r = r.numpy()
        np.testing.assert_allclose(a.cpu().numpy(), r, rtol=2e-4, atol=2e-4 * np.abs(r).max(), err_msg=name)


# ------------------------------------------------------------------ latent head

@pytest.mark.parametrize("case", C.HEAD_CASES, ids=lambda c: f"{c['b']}-{c['Ls']}-{c['Lg']}")
def test_latent_head_full_half_wave_and_second_sum_trip(ops, case):
    """ops.latent_head with all 32 lanes of a row in use, Ls > Lg, a single element, and 257 workgroups (second trip of the
    last workgroup's sum over the partials): the sample, both scalars and all three gradients against the fp64 formulas;
    the 257-workgroup sum is in a fixed order, so two launches give the same bits."""
    b, Ls, Lg = case["b"], case["Ls"], case["Lg"]
    zg, p_m, p_v, eps, gl = C.head_inputs(b, Ls, Lg)
    ref = C.latent_head_ref(zg, p_m, p_v, eps, gl, Ls, Lg)
    wk, wa = C.HEAD_WEIGHTS
    runs = []
    for _ in range(2 if case["sum_trips"] > 1 else 1):
        zd = zg.to(DEV, torch.float32).requires_grad_(True)
        pmd, pvd = (t.to(DEV).requires_grad_(True) for t in (p_m, p_v))
        lat, kl_d, al_d = ops.latent_head(zd, pmd, pvd, eps.to(DEV, torch.float32), Ls, Lg)
        ((lat * gl.to(DEV, torch.float32)).sum() + wk * kl_d + wa * al_d).backward()
        runs.append((lat.detach().clone(), kl_d.detach().clone(), al_d.detach().clone(), zd.grad, pmd.grad, pvd.grad))
    lat, kl_d, al_d, g_zg, g_pm, g_pv = runs[0]
    print(f"kl {float(kl_d)!r} ref {ref['kl']!r}; alignment {float(al_d)!r} ref {ref['al']!r}")
    np.testing.assert_allclose(lat.cpu().numpy(), ref["latent"].numpy(), rtol=2e-6, atol=2e-6)
    assert float(kl_d) == pytest.approx(ref["kl"], rel=1e-5) and float(al_d) == pytest.approx(ref["al"], rel=1e-5)
    for name, d, r in (("zg", g_zg, ref["zg"]), ("p_m", g_pm, ref["p_m"]), ("p_v", g_pv, ref["p_v"])):
        r = r.numpy()
        np.testing.assert_allclose(d.cpu().numpy(), r, rtol=1e-4, atol=1e-5 * np.abs(r).max(), err_msg=name)
    for other in runs[1:]:
        assert all(torch.equal(a, o) for a, o in zip(runs[0], other))


# ------------------------------------------------------------------ cluster losses

@pytest.mark.parametrize("case", C.CLUSTER_CASES, ids=lambda c: f"{c['b']}-{c['D']}-{c['K']}-{c['Kp']}")
def test_cluster_losses_chunks_general_path_and_slots(ops, case):
    """ops.cluster_losses with more than one chunk, on the general path (K > 16, or K * D > 512), with (cluster, column) pairs
    in slots 1..3, with the first chunk's overflow loop, Kp != K and a chunk larger than the batch: the saved counts, labels
    and batch means (read from the C entry's work buffer), both values, the gradient, the K-means term alone, and
    cluster_losses_fb -- the bits of forward + backward where the fused launch serves the shape, None elsewhere."""
    b, D, K, Kp = case["b"], case["D"], case["K"], case["Kp"]
    inp = C.cluster_inputs(case)
    ref = C.cluster_reference(inp)
    Kl = len(inp["clusters"])
    args = (i64(inp["all_labels"]), i64(inp["seeds"]), f32(inp["centres"]), f32(inp["prev"]), f32(inp["g_norm"]), i64(inp["clusters"]))
    # what the forward saves for the backward: means [K*D] | counts [K] | distinct labels | labels [b]
    zc = f32(inp["z"])
    out = torch.empty(2, dtype=torch.float32, device=DEV)
    work = torch.full((K * D + K + 1 + b,), float("nan"), dtype=torch.float32, device=DEV)
    rc = ops.model_lib().spadot_cluster_losses_forward(zc.data_ptr(), *(a.data_ptr() for a in args), b, D, K, Kp, Kl, 1, 1,
                                                       out.data_ptr(), work.data_ptr(), _stream())
    assert rc == 0
    wk = work.cpu().numpy().astype(np.float64)
    means, counts, nd, labels = wk[:K * D].reshape(K, D), wk[K * D:K * D + K], wk[K * D + K], wk[K * D + K + 1:]
    bad = np.nonzero(counts != ref["counts"])[0]
    print(f"km {float(out[0])!r} ref {ref['km']!r}; ot {float(out[1])!r} ref {ref['ot']!r}; distinct {nd} ref {(ref['counts'] > 0).sum()}; "
          f"clusters with a wrong count {bad.tolist()}: got {counts[bad].tolist()} ref {ref['counts'][bad].tolist()}; "
          f"max |mean - ref| {np.abs(means - ref['means']).max():.3e}")
    assert np.array_equal(counts, ref["counts"]) and nd == (ref["counts"] > 0).sum() and np.array_equal(labels, ref["labels"])
    # a mean is an fp32 sum of n rows in a fixed order, divided once: |error| <= n 2**-24 max |z|
    np.testing.assert_allclose(means, ref["means"], rtol=0, atol=ref["counts"].max() * 2.0 ** -24 * np.abs(inp["z"]).max())
    # values and gradient
    w_km, w_ot = C.CLUSTER_WEIGHTS
    zd = f32(inp["z"]).requires_grad_(True)
    km, ot = ops.cluster_losses(zd, *args, True, True)
    (w_km * km + w_ot * ot).backward()
    assert float(km) == float(out[0]) and float(ot) == float(out[1])
    assert float(km) == pytest.approx(ref["km"], rel=2e-5) and float(ot) == pytest.approx(ref["ot"], rel=2e-5)
    print(f"dz: worst |err| / (2e-4 |ref| + 2e-6 max |ref|) = {worst_ratio(zd.grad.cpu().numpy(), ref['dz'], 2e-4, 2e-6 * np.abs(ref['dz']).max()):.3f}")
    np.testing.assert_allclose(zd.grad.cpu().numpy(), ref["dz"], rtol=2e-4, atol=2e-6 * np.abs(ref["dz"]).max())
    # the K-means term alone (the switch of the first epochs)
    km1, ot1 = ops.cluster_losses(zd.detach(), args[0], args[1], args[2], do_km=True, do_ot=False)
    assert float(km1) == float(km) and float(ot1) == 0.0
    # forward + gradient in one launch
    wv = torch.tensor([w_km, w_ot], dtype=torch.float32, device=DEV)
    for do_km, do_ot in ((True, True), (True, False)):
        zp = f32(inp["z"]).requires_grad_(True)
        kmp, otp = ops.cluster_losses(zp, *args, do_km, do_ot)
        torch.autograd.backward([kmp, otp], [wv[0], wv[1]])
        zq = f32(inp["z"]).requires_grad_(True)
        res = ops.cluster_losses_fb(zq, *args, do_km, do_ot, wv[0], wv[1])
        if not case["fb"]:                    # outside the fused launch's range (-95): the caller falls back
            assert res is None
            continue
        kmq, otq, dzq = res
        assert float(kmq) == float(kmp) and float(otq) == float(otp)
        assert torch.equal(dzq, zp.grad)
