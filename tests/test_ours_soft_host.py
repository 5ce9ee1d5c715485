"""SGFormerSOFT (sgformer_amd/ours_soft.py, the drop-in for medium/ablation/oursSOFT.py) without a GPU, on a CPU kernel table
that has the pair_softmax_* entries: state_dict keys, logits and parameter gradients against the fixtures
tests/golden/soft/soft_cfg{0,1}.npz (scripts/make_soft_golden.py: the live reference in fp64).

The fixtures hold two recordings.  `logits` / `grad/*` are the reference exactly as shipped, whose F.softmax(scores [N, L, H],
dim=-1) normalises over the heads: the module as constructed (softmax_over = 'heads') meets it, in plain PyTorch, whatever
SGF_PAIR_SOFTMAX says.  `logits_keys` / `grad_keys/*` are the reference's code with that call taken over the keys, the exact
softmax attention of include/sgf.h block N8: the module after set_softmax_over('keys') meets it on the kernels' entries
(SGF_PAIR_SOFTMAX=1) and on the dense path (=0).  The two recordings differ by max |logits| 3.14 (cfg0, H = 1: the shipped weights
are all 1 and the layer returns the sum of the value rows) and 0.459 (cfg1, H = 2)."""
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.cpu_kernels_pair_softmax import CpuKernelsPairSoftmax  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "soft", "soft_cfg*.npz")))
LOGITS_BAR, GRAD_TOL = 1e-4, 1e-3               # the fp32 bars of tests/test_gpu_pair_softmax.py


class _Data:
    def __init__(self, x, ei):
        self.graph = {"node_feat": x, "edge_index": ei}


def load_fixture(path):
    """(meta, state, x, edge_index, y, {recording: (logits, grads)}) as torch tensors"""
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    pick = lambda prefix: {k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}      # noqa: E731
    rec = {"keys": (torch.from_numpy(z["logits_keys"]), pick("grad_keys/")), "shipped": (torch.from_numpy(z["logits"]), pick("grad/"))}
    return meta, pick("state/"), torch.from_numpy(z["x"]), torch.from_numpy(z["edge_index"]), torch.from_numpy(z["y"]), rec


def build_model(meta, over="heads"):
    """the fixture's model; over = 'heads' is the module as constructed"""
    from sgformer_amd import ours_medium, ours_soft
    gnn = None
    if meta["use_graph"]:
        gnn = ours_medium.GCN(meta["in_channels"], meta["hidden_channels"], meta["hidden_channels"], num_layers=meta["gcn_layers"],
                              dropout=0.0)
    m = ours_soft.SGFormerSOFT(meta["in_channels"], meta["hidden_channels"], meta["out_channels"], num_layers=meta["num_layers"],
                               num_heads=meta["num_heads"], dropout=0.0, use_weight=meta["use_weight"],
                               use_graph=meta["use_graph"], gnn=gnn)
    assert all(c.softmax_over == "heads" for c in m.trans_conv.convs)          # as constructed: the reference as shipped
    return m if over == "heads" else m.set_softmax_over(over)


def run_step(m, x, ei, y):
    m.train()
    logits = m(_Data(x, ei))
    torch.nn.functional.cross_entropy(logits.float(), y).backward()
    return logits.detach().double().cpu(), {k: p.grad.detach().double().cpu() for k, p in m.named_parameters() if p.grad is not None}


def compare(tag, logits, grads, ref_logits, ref_grads, logits_bar, grad_tol):
    """the worst error / bar over the logits (elementwise, bar * max(1, max|ref|)) and every gradient (||err|| against
    tol (||ref|| + 1e-2 gmax)); prints every ratio"""
    worst = float((logits - ref_logits.double()).abs().max()) / (logits_bar * max(1.0, float(ref_logits.abs().max())))
    print(f"SOFT_RATIO {tag}.logits {worst:.4f}")
    assert set(grads) == set(ref_grads), tag
    gmax = max(float(g.double().norm()) for g in ref_grads.values())
    for k, g in ref_grads.items():
        r = float((grads[k] - g.double()).norm()) / (grad_tol * (float(g.double().norm()) + 1e-2 * gmax))
        print(f"SOFT_RATIO {tag}.{k} {r:.4f}")
        worst = max(worst, r)
    return worst


@pytest.fixture
def table():
    from sgformer_amd import ops
    CpuKernelsPairSoftmax.calls = {}
    prev = ops.set_kernels(CpuKernelsPairSoftmax())
    yield CpuKernelsPairSoftmax
    ops.set_kernels(prev)


def test_there_are_two_fixtures():
    assert [os.path.basename(p) for p in FIXTURES] == ["soft_cfg0.npz", "soft_cfg1.npz"]
    metas = [load_fixture(p)[0] for p in FIXTURES]
    assert (metas[0]["num_heads"], metas[0]["use_weight"], metas[0]["use_graph"]) == (1, True, False)
    assert (metas[1]["num_heads"], metas[1]["use_weight"], metas[1]["use_graph"]) == (2, False, True)
    for p in FIXTURES:
        assert os.path.getsize(p) < 512 * 1024


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_state_dict_keys_are_the_reference_s(path):
    meta, state, *_ = load_fixture(path)
    own = build_model(meta).state_dict()
    assert list(own) == list(state)                                    # names AND creation order
    for k, v in state.items():
        assert tuple(own[k].shape) == tuple(v.shape), k


def test_constructor_signatures_are_the_reference_s():
    import inspect
    from sgformer_amd import ours_soft as S
    sig = lambda f: [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]      # noqa: E731
    assert sig(S.SGFormerSOFT.__init__) == [
        ("in_channels", inspect._empty), ("hidden_channels", inspect._empty), ("out_channels", inspect._empty), ("num_layers", 2),
        ("num_heads", 1), ("alpha", 0.5), ("dropout", 0.5), ("use_bn", True), ("use_residual", True), ("use_weight", True),
        ("use_graph", True), ("use_act", False), ("graph_weight", 0.8), ("gnn", None), ("aggregate", "add")]
    assert sig(S.TransConv.__init__) == [
        ("in_channels", inspect._empty), ("hidden_channels", inspect._empty), ("num_layers", 2), ("num_heads", 1), ("alpha", 0.5),
        ("dropout", 0.5), ("use_bn", True), ("use_residual", True), ("use_weight", True), ("use_act", False)]
    assert sig(S.TransConvLayer.__init__) == [("in_channels", inspect._empty), ("out_channels", inspect._empty),
                                              ("num_heads", inspect._empty), ("use_weight", True)]
    assert [n for n, _ in sig(S.TransConvLayer.forward)][:5] == ["query_input", "source_input", "edge_index", "edge_weight",
                                                                  "output_attn"]
    assert [n for n, _ in sig(S.softmax_attention)][:3] == ["ks", "vs", "output_attn"]
    m = S.SGFormerSOFT(8, 32, 3, gnn=None, use_graph=False)
    assert isinstance(m.trans_conv, S.TransConv) and all(isinstance(c, S.TransConvLayer) for c in m.trans_conv.convs)
    assert len(m.params1) == len(list(m.trans_conv.parameters())) and len(m.params2) == 2


@pytest.mark.parametrize("switch", ["1", "0"])
@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_matches_the_reference_with_the_softmax_over_the_keys(table, monkeypatch, path, switch):
    meta, state, x, ei, y, rec = load_fixture(path)
    monkeypatch.setenv("SGF_PAIR_SOFTMAX", switch)
    m = build_model(meta, "keys")
    m.load_state_dict(state)
    logits, grads = run_step(m, x, ei, y)
    layers = meta["num_layers"]
    want = {"pair_softmax_fwd": [meta["n"]] * layers, "pair_softmax_bwd_q": [meta["n"]] * layers,
            "pair_softmax_bwd_kv": [meta["n"]] * layers} if switch == "1" else {}
    assert table.calls == want
    assert compare(f"host[{os.path.basename(path)},switch{switch}]", logits, grads, *rec["keys"], LOGITS_BAR, GRAD_TOL) <= 1.0


@pytest.mark.parametrize("switch", ["1", "0"])
@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_matches_the_reference_as_shipped(table, monkeypatch, path, switch):
    """The module as constructed: the shipped reference's softmax over the heads, on no pair_softmax_* entry under either switch."""
    meta, state, x, ei, y, rec = load_fixture(path)
    monkeypatch.setenv("SGF_PAIR_SOFTMAX", switch)
    m = build_model(meta)
    m.load_state_dict(state)
    logits, grads = run_step(m, x, ei, y)
    assert table.calls == {}
    assert compare(f"host[{os.path.basename(path)},shipped]", logits, grads, *rec["shipped"], LOGITS_BAR, GRAD_TOL) <= 1.0


def test_attention_maps_and_other_shapes_stay_dense(table, monkeypatch):
    from sgformer_amd import ours_soft as S
    monkeypatch.setenv("SGF_PAIR_SOFTMAX", "1")
    meta, state, x, ei, y, _ = load_fixture(FIXTURES[1])
    m = build_model(meta, "keys")
    m.load_state_dict(state)
    with torch.no_grad():
        att = m.get_attentions(x)
    assert att.shape == (meta["num_layers"], meta["n"], meta["n"]) and table.calls == {}
    assert float((att.sum(2) - 1).abs().max()) <= 1e-5                  # rows of a softmax over the keys, averaged over the heads
    with torch.no_grad():
        att = m.set_softmax_over("heads").get_attentions(x)
    assert float((att - 1.0 / meta["num_heads"]).abs().max()) <= 1e-6   # as shipped: the weights of a pair sum to 1 over the heads
    torch.manual_seed(2)
    q, k, v = torch.randn(30, 2, 32), torch.randn(17, 2, 32), torch.randn(17, 2, 32)
    S.softmax_attention(q, k, v)                                        # the default axis: the heads, no kernel
    assert table.calls == {}
    out = S.softmax_attention(q, k, v, over="keys")
    assert table.calls == {"pair_softmax_fwd": [30]}
    out2, attn = S.softmax_attention(q, k, v, output_attn=True, over="keys")
    assert attn.shape == (30, 17) and table.calls == {"pair_softmax_fwd": [30]}
    assert float((out - out2).abs().max()) <= 1e-6
    S.softmax_attention(q, k, v, over="keys", shard=object())          # the node-sharded case
    S.softmax_attention(q[:, :, :24], k[:, :, :24], v, over="keys")     # a width the kernels do not take
    assert table.calls == {"pair_softmax_fwd": [30]}
    with pytest.raises(ValueError, match="over"):
        S.softmax_attention(q, k, v, over="queries")
    with pytest.raises(ValueError, match="over"):
        m.set_softmax_over("queries")
