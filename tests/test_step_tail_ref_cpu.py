"""CPU checks of tests/step_tail_cases.py: the fp64 clip + AdamW reference against torch, and every edge case against
the branch it is there for -- derived here from the recorded geometry constants and the case's shape, so that a case
which no longer reaches its branch fails on the CPU instead of passing quietly on the GPU."""
import numpy as np
import pytest
import torch

import step_tail_cases as C

G = C.GEOM
cdiv = lambda a, b: -(-a // b)


# ----------------------------------------------------------------------------------------------- clip + AdamW reference
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
def test_clip_adamw_ref_equals_torch_clip_and_adamw_in_fp64(grad_scale):
    """4 steps, clipped and unclipped in turn.  With grad_scale the buffer stands for grad_scale * g: the reference on g
    equals torch on grad_scale * g."""
    rng = np.random.default_rng(0)
    shapes = [(7, 13), (13,), (5, 3, 2), (1,)]
    lr, betas, eps, wd, max_norm = 3e-3, (0.9, 0.999), 1e-8, 1e-2, 0.3
    p0 = [rng.normal(size=s) for s in shapes]
    tp = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in p0]
    opt = torch.optim.AdamW(tp, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p, m, v = p0, [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
    clipped = []
    for step in range(4):
        g = [rng.normal(size=s) * (3.0 if step % 2 else 0.01) / grad_scale for s in shapes]
        for q, gr in zip(tp, g):
            q.grad = torch.tensor(gr * grad_scale, dtype=torch.float64)
        total = float(torch.nn.utils.clip_grad_norm_(tp, max_norm))
        opt.step()
        p, m, v, sumsq = C.clip_adamw_ref(p, g, m, v, step + 1, lr, betas, eps, wd, max_norm, grad_scale)
        clipped.append(total > max_norm)
        assert np.sqrt(sumsq) * grad_scale == pytest.approx(total, rel=1e-12)
        for q, a, mm, vv in zip(tp, p, m, v):
            st = opt.state[q]
            np.testing.assert_allclose(a, q.detach().numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(mm, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(vv, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
    assert clipped == [False, True, False, True]


def test_clip_adamw_ref_takes_one_array_and_leaves_its_inputs():
    rng = np.random.default_rng(1)
    p, g, m, v = (rng.normal(size=9) for _ in range(4))
    v = np.abs(v)
    keep = [a.copy() for a in (p, g, m, v)]
    one = C.clip_adamw_ref(p, g, m, v, 3, 1e-3, (0.9, 0.999), 1e-8, 1e-2, 0.3, 0.5)
    lst = C.clip_adamw_ref([p[:4], p[4:]], [g[:4], g[4:]], [m[:4], m[4:]], [v[:4], v[4:]], 3, 1e-3, (0.9, 0.999), 1e-8, 1e-2, 0.3, 0.5)
    for a, b in zip(one[:3], lst[:3]):
        np.testing.assert_allclose(a, np.concatenate(b), rtol=1e-15)
    assert one[3] == pytest.approx(lst[3], rel=1e-15)
    for a, b in zip((p, g, m, v), keep):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------------------------- the cases reach their branches
@pytest.mark.parametrize("case", C.SUMSQ_CASES, ids=lambda c: str(c["count"]))
def test_sumsq_case_reaches_its_branch(case):
    count = case["count"]
    n4 = count // 4
    wgs = min(max(cdiv(n4, G["wg"]), 1), G["sumsq_cap"])
    stride = wgs * G["wg"]
    assert case["n4"] == n4 and case["wgs"] == wgs and case["tail"] == count % 4
    assert case["lanes"] == min(G["sumsq_unroll"], cdiv(n4, stride))
    assert case["trips"] == cdiv(n4, G["sumsq_unroll"] * stride)
    assert case["final_trips"] == cdiv(wgs, G["final_sum_threads"])
    assert wgs <= 4096                      # FlatAdamW.scratch: one double per workgroup


def test_sumsq_cases_cover_the_branches():
    by = lambda key: {c[key] for c in C.SUMSQ_CASES}
    assert {0, 1, 2, 4} <= by("lanes") and {0, 1, 2} <= by("trips") and {1, 2} <= by("final_trips") and {1, 2, 3} <= by("tail")
    assert any(c["n4"] == 0 for c in C.SUMSQ_CASES) and any(c["n4"] == G["wg"] for c in C.SUMSQ_CASES)
    g = C.sumsq_values(1027)
    mag = np.abs(g.astype(np.float64))
    assert g.dtype == np.float32 and mag.max() / mag.min() > 3e3 and (g > 0).any() and (g < 0).any()


def test_adamw_case_reaches_its_branches():
    case = C.ADAMW_CASE
    sizes = [int(np.prod(s)) for s in case["shapes"]]
    padded = sum(cdiv(s, 4) * 4 for s in sizes)
    assert padded == case["padded"] == 8397836
    n4 = padded // 4
    sum_stride = G["sumsq_cap"] * G["wg"]
    assert cdiv(n4, G["sumsq_unroll"] * sum_stride) == case["sumsq_trips"] == 2
    assert (n4 > G["adamw_cap"] * G["wg"]) is case["img_strides"] is True          # k_adamw_img under step()
    assert padded > G["adamw_cap"] * G["wg"]                                        # k_adamw under step() without images
    # step_head() / step_rest(): `first` at the start, `last` at the end, each range past the range entry's grid
    head = sum(cdiv(sizes[i], 4) * 4 for i in case["first"])
    assert head == case["head_count"]
    for rng_len in (head, padded - head):
        assert (rng_len // 4 > G["range_cap"] * G["wg"]) is case["range_strides"] is True
    # the images: matrices with K % 4 == 0, one with pad columns, one inside the `first` group, one past it (base > 0)
    for i, Kp in case["images"].items():
        rows, K = case["shapes"][i]
        assert K % 4 == 0 and Kp % 4 == 0 and Kp >= K and rows * K < 2 ** 31
    assert any(Kp > case["shapes"][i][1] for i, Kp in case["images"].items())
    assert set(case["first"]) & set(case["images"]) and set(case["images"]) - set(case["first"])
    assert any(s % 4 for s in sizes)                                                # padding between segments
    # the three steps: clipped, unclipped, and a clipped one behind grad_scale (norm ~ sigma sqrt(count))
    n = sum(sizes)
    for st in case["steps"]:
        norm = st["sigma"] * float(np.sqrt(n)) * st["grad_scale"]
        assert (norm > 2 * case["max_norm"]) == st["clipped"] and (st["clipped"] or norm < 0.5 * case["max_norm"])
    assert [st["grad_scale"] for st in case["steps"]] == [1.0, 1.0, 0.25] and case["step0"] == 20000
    assert case["steps"][2]["sigma"] == 4 * case["steps"][0]["sigma"]


@pytest.mark.parametrize("case", C.BN_CASES, ids=lambda c: f"{c['b']}-{c['F']}")
def test_bn_case_reaches_its_branch(case):
    assert case["path"] == ("register" if case["b"] <= G["bn_rows"] else "looped")
    assert case["wgs"] == cdiv(case["F"], G["bn_cols"]) and case["idle_cols"] == case["wgs"] * G["bn_cols"] - case["F"]


def test_bn_cases_cover_the_branches():
    looped = [c for c in C.BN_CASES if c["path"] == "looped"]
    assert {c["dtype"] for c in looped} == {"float32", "bfloat16"} and any(not c["bias"] for c in looped)
    assert any(c["b"] == G["bn_rows"] + 1 for c in looped) and any(c["b"] % G["bn_rg"] for c in looped)
    assert any(c["b"] < G["bn_rg"] for c in C.BN_CASES) and any(c["F"] == 1 for c in C.BN_CASES)


@pytest.mark.parametrize("case", C.LN_CASES, ids=lambda c: f"{c['b']}-{c['F']}")
def test_ln_case_reaches_its_branch(case):
    b, F = case["b"], case["F"]
    assert case["row_wgs"] == cdiv(b, G["ln_rows_per_wg"]) and case["last_rows"] == (b % G["ln_rows_per_wg"] or G["ln_rows_per_wg"])
    assert case["idle_lanes"] == max(0, 64 - F)
    assert case["col_trips"] == cdiv(b, G["ln_rg"]) and case["col_wgs"] == cdiv(F, G["bn_cols"]) and case["ragged"] == F % G["bn_cols"]


def test_ln_cases_cover_the_branches():
    assert any(c["idle_lanes"] > 0 and c["F"] > 1 for c in C.LN_CASES)                           # F < 64
    assert any(c["ragged"] and c["col_trips"] > 1 and c["F"] > 64 for c in C.LN_CASES)          # F % 16 != 0 with b > LN_RG
    assert any(c["last_rows"] != G["ln_rows_per_wg"] and c["row_wgs"] > 1 for c in C.LN_CASES)   # b % 4 != 0, several workgroups
    assert any(c["F"] == 1 for c in C.LN_CASES)


@pytest.mark.parametrize("case", C.HEAD_CASES, ids=lambda c: f"{c['b']}-{c['Ls']}-{c['Lg']}")
def test_head_case_reaches_its_branch(case):
    wgs = cdiv(case["b"], G["head_rows_per_wg"])
    assert case["wgs"] == wgs and case["sum_trips"] == cdiv(wgs, G["head_sum_stride"]) and case["lanes"] == case["Ls"] + case["Lg"] <= 32


def test_head_cases_cover_the_branches():
    assert any(c["lanes"] == 32 for c in C.HEAD_CASES) and any(c["Ls"] > c["Lg"] for c in C.HEAD_CASES)
    assert any(c["sum_trips"] == 2 for c in C.HEAD_CASES) and any(c["b"] == 1 for c in C.HEAD_CASES)


def _cluster_geometry(b, D, K, Kp, Kl):
    chunk = min(G["cl_chunk_floats"] // D, b)
    chunk = cdiv(max(chunk, G["cl_min_chunk"]), 8) * 8
    fast = K <= G["cl_kreg"] and K * D <= G["cl_threads"]
    part = (G["cl_threads"] // D) * K * (D + 1)                       # the fast path's segment partials, reused by the fused gradient
    return {"chunk": chunk, "chunks": cdiv(b, chunk), "path": "fast" if fast else "general",
            "slots": cdiv(K * D, G["cl_threads"]), "overflow": min(chunk, b) * D > G["cl_zb"] * G["cl_threads"],
            "fb": fast and chunk >= b and part >= 2 * K * D + Kp * Kl}


@pytest.mark.parametrize("case", C.CLUSTER_CASES, ids=lambda c: f"{c['b']}-{c['D']}-{c['K']}")
def test_cluster_case_reaches_its_branch_and_has_its_edges(case):
    inp = C.cluster_inputs(case)
    b, D, K, Kp = case["b"], case["D"], case["K"], case["Kp"]
    Kl = len(inp["clusters"])
    geo = _cluster_geometry(b, D, K, Kp, Kl)
    assert {k: case[k] for k in geo} == geo
    assert K <= G["cl_maxk"] and Kp <= G["cl_maxk"] and D <= 64
    lab = inp["all_labels"][inp["seeds"]]
    assert inp["seeds"].size == b == np.unique(inp["seeds"]).size and lab.min() >= 0 and lab.max() < K
    assert Kl == K - 1 and C.CLUSTER_ABSENT_TIMEPOINT not in inp["clusters"]              # one cluster missing from the time point
    assert C.CLUSTER_ABSENT_BATCH in inp["clusters"] and not (lab == C.CLUSTER_ABSENT_BATCH).any()      # one missing from the batch
    assert not inp["g_norm"][C.CLUSTER_DEAD_ROW].any() and inp["g_norm"].sum(1).round(9).tolist().count(1.0) == Kp - 1
    ref = C.cluster_reference(inp)
    assert ref["counts"].sum() == b and ref["counts"][C.CLUSTER_ABSENT_BATCH] == 0
    assert np.array_equal(ref["means"][C.CLUSTER_ABSENT_BATCH], inp["centres"][C.CLUSTER_ABSENT_BATCH])
    assert np.isfinite(ref["dz"]).all() and ref["km"] > 0 and ref["ot"] > 0


def test_cluster_cases_cover_the_branches():
    cs = C.CLUSTER_CASES
    fast, gen = [c for c in cs if c["path"] == "fast"], [c for c in cs if c["path"] == "general"]
    assert any(c["chunks"] == 2 and c["b"] % c["chunk"] == 1 for c in fast)                # a second chunk of one row
    assert any(c["chunks"] >= 3 and c["Kp"] != c["K"] for c in fast) and any(c["overflow"] and c["chunks"] > 1 for c in fast)
    assert any(c["chunks"] == 1 for c in gen) and any(c["chunks"] >= 3 and c["slots"] == 2 for c in gen)
    assert any(c["K"] == c["Kp"] == G["cl_maxk"] and c["slots"] == 4 for c in gen)
    assert any(c["K"] * c["D"] == G["cl_threads"] and c["fb"] for c in fast)               # the last legal fast-path size
    assert any(c["K"] <= G["cl_kreg"] and c["K"] * c["D"] > G["cl_threads"] for c in gen)   # K small, K * D past slot 0
    assert any(c["b"] < G["cl_min_chunk"] for c in cs) and any(c["K"] == G["cl_kreg"] + 1 for c in gen)
    assert any(not c["fb"] and c["path"] == "fast" for c in cs)
