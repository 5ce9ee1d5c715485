"""The split-bf16 arm of the all-pair attention on the GPU: fp32 tensors under torch.set_float32_matmul_precision('high') through
sgformer_amd/pair_attn.py onto the sgf_pair_*_x3_* entries (csrc/pair_attn.hip, include/sgf.h block N9).

The reference is the dense formula in fp64 on the CPU.  The cases, their references and the bars are those of
tests/test_pair_x3_host.py (its docstring states the bars and where they come from), where an fp64 emulation of the arm's
arithmetic is held to half of each bar and the cross-term cases are shown to notice a dropped term.  The exact-mask and
cross-term cases are held to what tests/test_gpu_pair_attn.py / tests/test_gpu_pair_softmax.py ask of fp32 storage: their
operands make every product exact, so out is within one fp32 ulp of the masked mean, rowsum is the count, lse within one ulp,
and the gradients under the fp32 bars (1e-3).  Each check prints `X3_RATIO <name> <error / bar>` before it asserts
(pytest -s shows them; profiles/pair_x3_probe.md records the worst)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_gpu_pair_attn import _exact_case  # noqa: E402
from tests.test_ours_soft_host import FIXTURES, build_model, load_fixture, run_step  # noqa: E402
from tests.test_pair_x3_host import (ARMS, GRAD_TOL_X3, HEADS, RANDOM_SHAPES, SHAPES, V_LO_SHAPES, WIDTHS, cross_case,  # noqa: E402
                                     dense64, moving_case, precision, random_case, random_params, v_lo_case)

pytestmark = pytest.mark.gpu

F32X = 2
GRAD_TOL_F32 = 1e-3                # the fp32 gradient bar of the exact-arithmetic cases


def _ratio(name, err, bar):
    r = float(err) / float(bar) if bar > 0 else (0.0 if err == 0 else float("inf"))
    print(f"X3_RATIO {name} {r:.4f}")
    return r


def _lap_shapes(arm, d):
    """(n, l) at which a workgroup of one of the split kernels walks three tiles (none while every workgroup owns one tile)"""
    from sgformer_amd import _lib
    lap = getattr(_lib.load(), f"sgf_pair_{arm}_x3_lap_rows")
    rows = [int(lap(w, 3, d, F32X, 3)) for w in (0, 1, 2)]
    assert all(r >= 0 for r in rows)
    return [(r, 65) if w < 2 else (65, r) for w, r in enumerate(rows) if r > 0]


def _entries(arm, q, k, v, g, scale=1.0, p="high"):
    """(out, saved, dq, dk, dv) of the three launches under the matmul precision `p`, on tensors already on the GPU"""
    from sgformer_amd.pair_attn import _Hip
    with precision(p):
        if arm == "softmax":
            out, saved = _Hip.pair_softmax_fwd(q, k, v, scale)
            dq, delta = _Hip.pair_softmax_bwd_q(g, out, saved, q, k, v, scale)
            dk, dv = _Hip.pair_softmax_bwd_kv(g, saved, delta, q, k, v, scale)
        else:
            out, saved = _Hip.pair_sigmoid_fwd(q, k, v)
            dq, delta = _Hip.pair_sigmoid_bwd_q(g, out, saved, q, k, v)
            dk, dv = _Hip.pair_sigmoid_bwd_kv(g, saved, delta, q, k, v)
    torch.cuda.synchronize()
    return out, saved, dq, dk, dv


def _check_grads(tag, got, ref, tol):
    gmax = max(float(t.norm()) for t in ref)
    worst = 0.0
    for name, a, b in zip(("dq", "dk", "dv"), got, ref):
        worst = max(worst, _ratio(f"{tag}.{name}", (a.double().cpu() - b).norm(), tol * (float(b.norm()) + 1e-2 * gmax)))
    return worst


# ------------------------------------------------------------------------------------------------
# 1. and 2.  exact masks and the cross terms: every product exact
# ------------------------------------------------------------------------------------------------
_exact_grads = {}


def _check_exact(cuda, arm, tag, case, zmax=32.0, weight=1.0, wide=False):
    """the kept keys score zmax with a weight of exactly `weight` (sigmoid; the softmax's is 1 after the maximum), the others 0"""
    q, k, v, g, count, out_ref, dv_ref = case
    if (arm, tag) not in _exact_grads:
        _exact_grads[(arm, tag)] = dense64(arm, q, k, v, g)[2:5]
    grads_ref = _exact_grads[(arm, tag)]

    def dev(t):
        t = t.to(cuda, torch.float32)
        if not wide:
            return t
        buf = torch.full((t.shape[0], t.shape[1] * t.shape[2] + 24), 77.0, device=cuda, dtype=torch.float32)      # ld > H * D
        view = buf[:, 8:8 + t.shape[1] * t.shape[2]].view(t.shape[0], t.shape[1], t.shape[2])
        view.copy_(t)
        return view
    out, saved, dq, dk, dv = _entries(arm, dev(q), dev(k), dev(v), dev(g))
    tag = f"{tag}[{arm}{',wide' if wide else ''}]"
    if arm == "softmax":
        lse_ref = zmax + torch.log(count)
        err = (saved.double().cpu() - lse_ref).abs()
        ulp = 2.0 ** -23 * torch.exp2(torch.floor(torch.log2(lse_ref)))
        assert bool((err <= ulp).all()), (tag, "lse", float((err / ulp).max()))
    else:
        assert torch.equal(saved.double().cpu(), weight * count), (tag, "rowsum")
    err = (out.double().cpu() - out_ref).abs()
    ulp = 2.0 ** -23 * torch.exp2(torch.floor(torch.log2(out_ref.abs().clamp_min(1e-30))))
    assert bool((err <= ulp).all()), (tag, "out", float((err / ulp).max()))
    bar = GRAD_TOL_F32 * (1.0 + 1e-2) * float(dv_ref.norm())
    assert _ratio(tag + ".dv_masked_mean", (dv.double().cpu() - dv_ref).norm(), bar) <= 1.0, tag
    if arm == "sigmoid" and weight == 1.0:           # saturated: 1 - S is formed from S, dZ is exactly 0
        assert not bool(dq.abs().max() > 0) and not bool(dk.abs().max() > 0), tag
    assert _check_grads(tag, (dq, dk, dv), grads_ref, GRAD_TOL_F32) <= 1.0, tag


@pytest.mark.parametrize("h,hv", HEADS)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("arm", ARMS)
def test_exact_masks(cuda, arm, d, h, hv):
    for n, l in SHAPES + _lap_shapes(arm, d):
        _check_exact(cuda, arm, f"exact[{n}x{l},H{h},Hv{hv},D{d}]", _exact_case(n, l, h, hv, d))


@pytest.mark.parametrize("arm", ARMS)
def test_exact_masks_in_wider_buffers(cuda, arm):
    _check_exact(cuda, arm, "exact[70x193,H3,Hv3,D64]", _exact_case(70, 193, 3, 3, 64), wide=True)
    _check_exact(cuda, arm, "exact[257x255,H3,Hv1,D32]", _exact_case(257, 255, 3, 1, 32), wide=True)


@pytest.mark.parametrize("h,hv", HEADS)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("kind", ["q_lo", "k_lo"])
@pytest.mark.parametrize("arm", ARMS)
def test_score_cross_terms(cuda, arm, kind, d, h, hv):
    """z = 32 / -128 is carried by lo_q . hi_k (q_lo) or hi_q . lo_k (k_lo) alone, in the forward and in both backward launches,
    which recompute z: a kernel without that term returns the uniform average"""
    for n, l in SHAPES + _lap_shapes(arm, d):
        _check_exact(cuda, arm, f"{kind}[{n}x{l},H{h},Hv{hv},D{d}]", cross_case(kind, n, l, h, hv, d))


@pytest.mark.parametrize("h,hv", HEADS)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("arm", ARMS)
def test_value_cross_term(cuda, arm, d, h, hv):
    """out = 2^-10 mean_j t_jf is carried by P_hi . V_lo alone: a kernel without that term returns 0"""
    for n, l in V_LO_SHAPES:
        case = v_lo_case(n, l, h, hv, d)
        assert float(case[5].abs().min()) > 0.0
        _check_exact(cuda, arm, f"v_lo[{n}x{l},H{h},Hv{hv},D{d}]", case, zmax=0.0, weight=0.5)


# ------------------------------------------------------------------------------------------------
# 3. random operands that bf16 does not hold, against fp64
# ------------------------------------------------------------------------------------------------
def _check_parity(cuda, tag, case, grads=True):
    """forward and saved row value under their bars; the gradients under 2e-4 where `grads`, finite everywhere"""
    arm, q, k, v, g, scale, ref, bar = case
    got = _entries(arm, *(t.to(cuda, torch.float32) for t in (q, k, v, g)), scale)
    tag = f"{tag}[{arm},{q.shape[0]}x{k.shape[0]},H{q.shape[1]},Hv{v.shape[1]},D{q.shape[2]},s{scale}]"
    for t in got:
        assert bool(torch.isfinite(t).all()), tag
    worst = _ratio(tag + ".out", ((got[0].double().cpu() - ref[0]).abs() / bar[0]).max(), 1.0)
    worst = max(worst, _ratio(tag + ".saved", ((got[1].double().cpu() - ref[1]).abs() / bar[1]).max(), 1.0))
    gworst = _check_grads(tag, got[2:], ref[2:5], GRAD_TOL_X3)
    assert worst <= 1.0, tag
    assert not grads or gworst <= 1.0, tag


@pytest.mark.parametrize("arm,d,h,hv,scale", random_params())
def test_random_parity(cuda, arm, d, h, hv, scale):
    for n, l in RANDOM_SHAPES + _lap_shapes(arm, d):
        _check_parity(cuda, "random", random_case(arm, n, l, h, hv, d, scale), grads=scale == 0.125)


@pytest.mark.parametrize("arm", ARMS)
def test_large_and_moving_scores(cuda, arm):
    """scores to 640, 1280 and (softmax) 3000: the forward under its bar, every gradient finite"""
    _check_parity(cuda, "moving64", moving_case(arm, 64), grads=False)
    _check_parity(cuda, "moving32", moving_case(arm, 32), grads=False)
    _check_parity(cuda, "large", random_case(arm, 257, 255, 2, 2, 64, 1.0, zmax=3000.0 if arm == "softmax" else 30.0), grads=False)


def test_random_parity_in_a_wider_buffer(cuda):
    arm, q, k, v, g, scale, ref, bar = random_case("softmax", 70, 193, 3, 1, 64, 0.125)

    def dev(t):
        buf = torch.full((t.shape[0], t.shape[1] * t.shape[2] + 12), 77.0, device=cuda, dtype=torch.float32)
        view = buf[:, 4:4 + t.shape[1] * t.shape[2]].view(t.shape[0], t.shape[1], t.shape[2])
        view.copy_(t.to(cuda, torch.float32))
        return view
    got = _entries(arm, dev(q), dev(k), dev(v), dev(g), scale)
    assert float(((got[0].double().cpu() - ref[0]).abs() / bar[0]).max()) <= 1.0
    assert _check_grads("random_wide", got[2:], ref[2:5], GRAD_TOL_X3) <= 1.0


# ------------------------------------------------------------------------------------------------
# 4. the arm ran, and left nothing behind
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ARMS)
def test_the_split_arm_runs_under_high_only(cuda, arm):
    from sgformer_amd import _lib
    q, k, v, g = (t.to(cuda, torch.float32) for t in random_case(arm, 1031, 1031, 3, 3, 64, 0.125)[1:5])
    before = _entries(arm, q, k, v, g, 0.125, p="highest")
    high = _entries(arm, q, k, v, g, 0.125)
    again = _entries(arm, q, k, v, g, 0.125)
    after = _entries(arm, q, k, v, g, 0.125, p="highest")
    assert torch.get_float32_matmul_precision() == "highest"
    for name, a, b, c, e in zip(("out", "saved", "dq", "dk", "dv"), before, high, again, after):
        assert not torch.equal(a, b), (name, "the 'high' result is the 'highest' one: the split kernels did not run")
        assert torch.equal(b, c), (name, "two 'high' launches differ")
        assert torch.equal(a, e), (name, "'highest' changed after a 'high' call")
    lib = _lib.load()
    assert getattr(lib, f"sgf_pair_{arm}_supported")(3, 3, 64, F32X) == 0
    s = (0.125,) if arm == "softmax" else ()
    out, saved = torch.empty_like(q), torch.empty(1031, 3, device=cuda)
    rc = getattr(lib, f"sgf_pair_{arm}_fwd")(q.data_ptr(), 192, k.data_ptr(), 192, v.data_ptr(), 192, 1031, 1031, 3, 3, 64, F32X,
                                             *s, out.data_ptr(), 192, saved.data_ptr(), None)
    assert rc == -4 and lib.sgf_last_error().startswith(f"sgf_pair_{arm}_fwd:".encode())


# ------------------------------------------------------------------------------------------------
# 5. the modules under 'high'
# ------------------------------------------------------------------------------------------------
LOGITS_BAR, GRAD_REL, GRAD_FLOOR = 2e-4, 5e-3, 1e-6        # tests/test_gpu_f32_precision.py, the model fixtures under 'high'


def _record_launches(monkeypatch):
    from sgformer_amd import pair_attn
    names, launch = [], pair_attn._launch
    monkeypatch.setattr(pair_attn, "_launch", lambda dev, name, *a: (names.append(name), launch(dev, name, *a))[1])
    return names


def _check_module(tag, logits, grads, ref_logits, ref_grads):
    assert _ratio(tag + ".logits", (logits - ref_logits.double()).abs().max(), LOGITS_BAR) <= 1.0
    gmax = max(float(g.double().norm()) for g in ref_grads.values())
    assert set(grads) == set(ref_grads)
    for k, g in ref_grads.items():
        bar = GRAD_REL * float(g.double().norm()) + GRAD_FLOOR * gmax
        assert _ratio(f"{tag}.{k}", (grads[k] - g.double()).norm(), bar) <= 1.0, k


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_soft_module_matches_the_fixtures_under_high(cuda, monkeypatch, path):
    meta, state, x, ei, y, rec = load_fixture(path)
    monkeypatch.setenv("SGF_PAIR_SOFTMAX", "1")
    names = _record_launches(monkeypatch)
    m = build_model(meta, "keys")
    m.load_state_dict(state)
    with precision("high"):
        logits, grads = run_step(m.to(cuda), x.to(cuda, torch.float32), ei.to(cuda), y.to(cuda))
    layers = meta["num_layers"]
    assert sorted(names) == sorted([f"sgf_pair_softmax_x3_{w}" for w in ("fwd", "bwd_q", "bwd_kv")] * layers), names
    _check_module(f"soft_fixture[{os.path.basename(path)}]", logits, grads, *rec["keys"])


class _Data:
    def __init__(self, x, ei):
        self.graph = {"node_feat": x, "edge_index": ei}


def test_difformer_sigmoid_matches_its_dense_path_in_fp64_under_high(cuda, monkeypatch):
    from sgformer_amd import difformer as M, ops
    from tests.cpu_kernels import CpuKernels
    n, f = 1500, 40
    torch.manual_seed(5)
    state = M.DIFFormer(f, 64, 7, num_layers=2, num_heads=2, kernel='sigmoid').state_dict()
    x = torch.randn(n, f)
    src = torch.randint(0, n, (8 * n,))
    dst = (src + 1 + torch.randint(0, n - 1, (8 * n,))) % n
    ei = torch.stack([torch.cat([src, dst]), torch.cat([dst, src])])
    y = torch.randint(0, 7, (n,))

    def run(device, dtype):
        m = M.DIFFormer(f, 64, 7, num_layers=2, num_heads=2, kernel='sigmoid', dropout=0.0)
        m.load_state_dict(state)
        m = m.to(device, dtype).train()
        logits = m(_Data(x.to(device, dtype), ei.to(device)))
        torch.nn.functional.cross_entropy(logits, y.to(device)).backward()
        return logits.detach().double().cpu(), {k: p.grad.double().cpu() for k, p in m.named_parameters() if p.grad is not None}
    monkeypatch.setenv("SGF_PAIR_ATTN", "0")
    prev = ops.set_kernels(CpuKernels())                  # the module's dense path, in fp64 on the CPU
    try:
        ref, ref_g = run("cpu", torch.float64)
    finally:
        ops.set_kernels(prev)
    monkeypatch.setenv("SGF_PAIR_ATTN", "1")
    names = _record_launches(monkeypatch)
    with precision("high"):
        got, got_g = run(cuda, torch.float32)
    assert sorted(names) == sorted([f"sgf_pair_sigmoid_x3_{w}" for w in ("fwd", "bwd_q", "bwd_kv")] * 2), names
    _check_module("difformer", got, got_g, ref, ref_g)
