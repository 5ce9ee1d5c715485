"""What the model layer (the autograd operators of sgformer_amd/linear.py and ops.py, the modules of ours.py and its variants)
asks of the kernel table, pinned without a GPU: a recording wrapper around tests/cpu_kernels.CpuKernels is installed with
ops.set_kernels(), every case runs two training steps and one eval forward under a fixed torch.manual_seed, and what was
recorded is compared with tests/golden/model_trace.json:

  * every kernel-table call in order (K.check left out): the method name, shape / dtype (and strides of a view) of every
    tensor argument, every scalar argument;
  * every shard.all_reduce / shard.unsum with its element count (the cases with a shard: a one-process stand-in, identity
    collectives — tests/test_dist.py is the check on real process groups);
  * after each of the three phases, a SHA-256 of the bytes of the logits, one over all parameter gradients, one over all
    BatchNorm running buffers and one over every num_batches_tracked (one digest per group, over its tensors in name order
    with their names, to keep the golden file small; call sequences that repeat are stored once).

The packed-gather and captured-dropout arms need kernels the CPU table does not have (bn_apply_packed, dropout_dev): they
stay with tests/test_gpu_spmm_packed_model.py and tests/test_gpu_graphed*.py.

Row counts 256 and 1061: the BatchNorm statistics sample is min(n, 1024) rows, a power of two for both, so that the sample
mean has one bit pattern whether it is formed as sums / ns or sums * (1 / ns).  The run is single-threaded: a CPU reduction
split over threads has no fixed summation order.

`python tests/test_model_trace_host.py --write` regenerates the golden file from the code as it stands.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "model_trace.json")

from tests.cpu_kernels import CpuKernels  # noqa: E402
from tests.test_host import CONFIGS  # noqa: E402

_SHORT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float64: "f64", torch.int64: "i64", torch.int32: "i32",
          torch.bool: "b8", torch.uint8: "u8"}


def _fmt(v, depth=2):
    if isinstance(v, torch.Tensor):
        s = f"{_SHORT.get(v.dtype, str(v.dtype))}{list(v.shape)}"
        return s if v.is_contiguous() else f"{s}/s{list(v.stride())}"
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    if isinstance(v, torch.dtype):
        return _SHORT.get(v, str(v))
    if isinstance(v, (list, tuple)):
        return "[" + (", ".join(_fmt(w, depth - 1) for w in v) if depth else "...") + "]"
    return type(v).__name__


class Recording:
    """CpuKernels behind a log.  A method the CPU table lacks stays missing (hasattr is the product's rule)."""

    def __init__(self, log):
        self._table, self._log = CpuKernels(), log

    def __getattr__(self, name):
        attr = getattr(self._table, name)
        if not callable(attr) or name == "check":
            return attr

        def call(*args, **kwargs):
            shown = [_fmt(a) for a in args] + [f"{k}={_fmt(v)}" for k, v in sorted(kwargs.items())]
            self._log.append(f"{name}({', '.join(shown)})")
            return attr(*args, **kwargs)
        return call


class OneProcessShard:
    """What the operators and modules touch of dist.ShardContext, for ONE process holding every row: the collectives are
    identities, logged with their element counts."""
    local_graph = local_edges = reorder = False

    def __init__(self, n, log):
        self.n_global, self._log = n, log

    def all_reduce(self, t):
        self._log.append(f"shard.all_reduce({t.numel()})")
        return t

    def unsum(self, t):
        if t is not None:
            self._log.append(f"shard.unsum({t.numel()})")
        return t

    def repartition_for(self, edge_index):
        return None

    def graph_for(self, edge_index):
        from sgformer_amd import ops
        g = ops.graph_cache.get(edge_index, self.n_global)
        g.n_local = g.n
        return g

    def gather_chunks(self, d):
        return 1

    def all_gather_rows(self, x, async_op=False):
        return x


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def _case(variant="large", cfg="products", bf16=False, n=256, f=24, c=7, drop=0.0, bn=None, env=None, shard=False,
          x_grad=False, **flags):
    return dict(variant=variant, cfg=cfg, bf16=bf16, n=n, f=f, c=c, drop=drop, bn=bn, env=env or {}, shard=shard,
                x_grad=x_grad, flags=flags)


CASES = {
    # fp32 storage (hidden width 16): the general matrix-core Linear, sgf_colstats statistics, the unfused BatchNorm path
    "f32-arxiv": _case(cfg="arxiv"),
    "f32-products-1061": _case(n=1061),
    "f32-heads-cat": _case(cfg="heads_cat"),
    "f32-bare": _case(cfg="bare"),
    "f32-alpha": _case(cfg="alpha", n=1061),
    "f32-no-graph": _case(cfg="arxiv", use_graph=False),
    "f32-dropout": _case(cfg="arxiv", drop=0.5),
    "f32-f65": _case(cfg="arxiv", f=65),
    "f32-x-grad": _case(cfg="arxiv", x_grad=True),
    "f32-bn-cumulative": _case(cfg="arxiv", bn="cumulative"),
    "f32-bn-untracked": _case(cfg="arxiv", bn="untracked"),
    "f32-bn-f64": _case(bn="f64"),
    "f32-shard": _case(n=1061, shard=True),
    "f32-shard-arxiv-dropout": _case(cfg="arxiv", shard=True, drop=0.5),
    "f32-100m": _case(variant="100m", cfg="alpha"),
    "f32-medium": _case(variant="medium"),
    "f32-medium-cat-dropout": _case(variant="medium", cfg="cat", drop=0.5, n=1061),
    "f32-difformer": _case(variant="difformer"),
    # bf16 storage (hidden width 64): the streaming row kernels, both stems in one node, the fused GraphConv layers
    "bf16-products": _case(bf16=True),
    "bf16-products-1061": _case(bf16=True, n=1061),
    "bf16-100m": _case(variant="100m", bf16=True, n=1061),
    "bf16-arxiv": _case(cfg="arxiv", bf16=True),
    "bf16-bn-cumulative": _case(bf16=True, bn="cumulative"),
    "bf16-bn-untracked": _case(bf16=True, bn="untracked"),
    "bf16-bn-f64": _case(bf16=True, bn="f64"),
    "bf16-dropout": _case(bf16=True, drop=0.5, n=1061),
    "bf16-no-init": _case(bf16=True, gnn_use_init=False),
    "bf16-no-gnn-residual": _case(bf16=True, gnn_use_residual=False),
    "bf16-no-gnn-bn": _case(bf16=True, gnn_use_bn=False),
    "bf16-no-gnn-act": _case(bf16=True, gnn_use_act=False),
    "bf16-no-trans-bn": _case(bf16=True, trans_use_bn=False),
    "bf16-no-trans-residual": _case(bf16=True, trans_use_residual=False),
    "bf16-cat": _case(bf16=True, aggregate="cat"),
    "bf16-no-graph": _case(bf16=True, use_graph=False),
    "bf16-heads": _case(bf16=True, trans_num_heads=2, trans_num_layers=2),
    "bf16-x-grad": _case(bf16=True, x_grad=True),
    "bf16-f65": _case(bf16=True, f=65),
    "bf16-c72": _case(bf16=True, c=72),
    "bf16-c70": _case(bf16=True, c=70),
    "bf16-shard": _case(bf16=True, shard=True),
    "bf16-shard-1061": _case(bf16=True, shard=True, n=1061),
    "bf16-shard-dropout": _case(bf16=True, shard=True, drop=0.5),
    "bf16-shard-bn-cumulative": _case(bf16=True, shard=True, bn="cumulative"),
    "bf16-env-gcn-fused-0": _case(bf16=True, env={"SGF_GCN_FUSED": "0"}),
    "bf16-env-stem-fused-0": _case(bf16=True, env={"SGF_STEM_FUSED": "0"}),
    "bf16-env-stem-ln-fused-0": _case(bf16=True, env={"SGF_STEM_LN_FUSED": "0"}),
    "bf16-env-gcn-bwd-fused-1": _case(bf16=True, env={"SGF_GCN_BWD_FUSED": "1"}),
    "bf16-env-gcn-dx-acc-0": _case(bf16=True, env={"SGF_GCN_DX_ACC": "0"}),
    "bf16-env-gram-pair-0": _case(bf16=True, env={"SGF_GRAM_PAIR": "0"}),
}
SWITCHES = ("SGF_GCN_FUSED", "SGF_STEM_FUSED", "SGF_STEM_LN_FUSED", "SGF_GCN_BWD_FUSED", "SGF_GCN_DX_ACC", "SGF_GRAM_PAIR")


class _Data:
    def __init__(self, x, ei):
        self.graph = {"node_feat": x, "edge_index": ei}


def _build(case):
    """(model, call(x, ei) -> logits) for one case; parameters from torch's seeded initialisation."""
    from sgformer_amd import difformer, ours, ours_100m, ours_medium, synth
    d = 64 if case["bf16"] else 16
    f, c, p = case["f"], case["c"], case["drop"]
    cdt = torch.bfloat16 if case["bf16"] else None
    if case["variant"] in ("large", "100m"):
        cfg = dict(synth.RECIPES["ogbn-products"] if case["cfg"] == "products" else CONFIGS[case["cfg"]])
        cfg.update(case["flags"])
        if case["variant"] == "100m":
            cfg.setdefault("alpha", 0.5)
        cls = ours.SGFormer if case["variant"] == "large" else ours_100m.SGFormer
        m = cls(f, d, c, trans_dropout=p, gnn_dropout=p, compute_dtype=cdt, **cfg)
        return m, m
    if case["variant"] == "medium":
        cfg = dict(num_layers=2, num_heads=2, use_weight=False, aggregate="cat") if case["cfg"] == "cat" else \
            dict(num_layers=1, alpha=0.5, graph_weight=0.8)
        gnn = ours_medium.GCN(f, d, d, num_layers=3, dropout=p)
        m = ours_medium.SGFormer(f, d, c, dropout=p, gnn=gnn, **cfg)
    else:
        m = difformer.DIFFormer(f, d, c, dropout=p, num_layers=2, num_heads=1)
    return m, (lambda x, ei: m(_Data(x, ei)))


def _set_batchnorm(m, how):
    for bn in m.modules():
        if isinstance(bn, torch.nn.BatchNorm1d):
            if how == "cumulative":
                bn.momentum = None
            elif how == "untracked":
                bn.track_running_stats = False
                bn.running_mean = bn.running_var = bn.num_batches_tracked = None
            elif how == "f64":
                bn.running_mean, bn.running_var = bn.running_mean.double(), bn.running_var.double()


def _sha(named):
    """One SHA-256 over the bytes of the named tensors in the order given, names, dtypes and shapes included."""
    h = hashlib.sha256()
    for name, t in named:
        t = t.detach().contiguous()
        h.update(f"{name}:{_SHORT.get(t.dtype, str(t.dtype))}{list(t.shape)};".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


GROUPS = ("logits", "gradients", "running statistics", "num_batches_tracked")


def _digests(m, logits):
    """GROUPS: the logits, every parameter gradient, every BatchNorm running buffer, every num_batches_tracked."""
    buffers = [(k, b) for k, b in m.named_buffers() if b is not None]
    return [_sha([("logits", logits)]),
            _sha([(k, prm.grad) for k, prm in m.named_parameters() if prm.grad is not None]),
            _sha([(k, b) for k, b in buffers if "running_" in k]),
            _sha([(k, b) for k, b in buffers if "num_batches_tracked" in k])]


def run_case(case, monkeypatch):
    """[(calls, digests)] of the three phases: training step, training step, eval forward."""
    from sgformer_amd import dist, ops, synth
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in case["env"].items():
        monkeypatch.setenv(name, value)
    log = []
    threads = torch.get_num_threads()
    prev = ops.set_kernels(Recording(log))
    torch.set_num_threads(1)
    try:
        torch.manual_seed(7)
        n = case["n"]
        m, call = _build(case)
        _set_batchnorm(m, case["bn"])
        if case["shard"]:
            dist.shard_model(m, OneProcessShard(n, log))
        x = torch.randn(n, case["f"]).requires_grad_(case["x_grad"])
        ei = synth.synthetic_graph(n, 6.0, seed=5)
        y = torch.randint(0, case["c"], (n,))
        phases = []
        m.train()
        for _ in range(2):
            del log[:]
            logits = call(x, ei)
            torch.nn.functional.cross_entropy(logits.float(), y).backward()
            phases.append((list(log), _digests(m, logits)))
            with torch.no_grad():                     # a plain gradient step: the second step starts from other weights
                for prm in m.parameters():
                    if prm.grad is not None:
                        prm.sub_(prm.grad, alpha=0.05)
                        prm.grad = None
            x.grad = None
        m.eval()
        del log[:]
        with torch.no_grad():
            logits = call(x, ei)
        phases.append((list(log), _digests(m, logits)))
        return phases
    finally:
        torch.set_num_threads(threads)
        ops.set_kernels(prev)


def _load():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", list(CASES))
def test_trace_matches_the_golden_file(name, monkeypatch):
    golden = _load()
    table, want = golden["calls"], golden["cases"][name]
    for i, (calls, digests) in enumerate(run_case(CASES[name], monkeypatch)):
        phase = ("train step 1", "train step 2", "eval")[i]
        expected = [table[j] for j in golden["sequences"][want[i][0]]]
        first = next((k for k, (a, b) in enumerate(zip(calls, expected)) if a != b), min(len(calls), len(expected)))
        assert calls == expected, (f"{name}, {phase}: {len(calls)} calls for {len(expected)}; first difference at call {first}: "
                                   f"{calls[first:first + 1]} for {expected[first:first + 1]}")
        wrong = [g for g, a, b in zip(GROUPS, digests, want[i][1:]) if a != b]
        assert not wrong and len(want[i]) == 1 + len(GROUPS), f"{name}, {phase}: other bits in {wrong}"


def test_golden_file_holds_exactly_the_cases():
    assert sorted(_load()["cases"]) == sorted(CASES)


def test_arms_the_issue_names_are_reached():
    """The default backward arms (paired Gram inside the BatchNorm backward, the head's gradient left as the Gram operand),
    both statistics forms, the one-launch finalize and every collective site are in the pinned traces."""
    golden = _load()
    table = golden["calls"]

    def names(case):
        return {table[j].split("(")[0] for phase in golden["cases"][case] for j in golden["sequences"][phase[0]]}

    assert {"gram2_bn_bwd", "combine_fc_bwd_g", "bn_finalize", "stem_pair", "gcn_epilogue_cat", "gram_bn_bwd",
            "gram_ln_bwd"} <= names("bf16-products")
    assert "gcn_bn_bwd_dx" in names("bf16-env-gcn-bwd-fused-1") and "gcn_epilogue_dx2" in names("bf16-env-gcn-dx-acc-0")
    assert "colstats" in names("f32-arxiv") and "pad_rows" in names("f32-f65") and "dropout" in names("f32-dropout")
    assert {"shard.all_reduce", "shard.unsum"} <= names("bf16-shard") and "shard.all_reduce" in names("f32-shard")


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_model_trace_host.py --write")
    table, sequences, cases, total = {}, {}, {}, 0
    for name, case in CASES.items():
        with pytest.MonkeyPatch.context() as mp:
            phases = run_case(case, mp)
        total += sum(len(calls) for calls, _ in phases)
        # a phase: [index of its call sequence, one SHA-256 per entry of GROUPS]; sequences and calls are stored once each
        cases[name] = [[sequences.setdefault(tuple(table.setdefault(s, len(table)) for s in calls), len(sequences))] + digests
                       for calls, digests in phases]
    with open(GOLDEN, "w") as fh:
        fh.write('{"calls": [\n' + ",\n".join(json.dumps(s) for s in table) + '\n],\n"sequences": [\n'
                 + ",\n".join(json.dumps(list(q), separators=(",", ":")) for q in sequences) + '\n],\n"cases": {\n'
                 + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in cases.items()) + "\n}}\n")
    print(f"wrote {os.path.relpath(GOLDEN, ROOT)}: {len(cases)} cases, {total} calls ({len(table)} distinct, "
          f"{len(sequences)} distinct sequences)")
