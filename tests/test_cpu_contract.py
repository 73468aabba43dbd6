"""unast_amd.contract is the one home of the three-launch fp32-level contractions and of the version-keyed operand cache:
source-level checks that nothing grows a second copy, and the refusals of a caller's `out` / `work` before any launch.  No GPU."""
import ast
import glob
import os

import pytest
import torch

from tests import rnn_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unast_amd")
MODULES = sorted(glob.glob(os.path.join(PKG, "*.py")))


def _tree(path):
    return ast.parse(open(path).read(), path)


def test_operand_parts_are_split_in_one_module():
    callers = [os.path.basename(p) for p in MODULES if "split_parts(" in open(p).read() and os.path.basename(p) != "ops.py"]
    assert callers == ["contract.py"], callers
    assert "ops.split_parts(" in open(os.path.join(PKG, "contract.py")).read()


def test_no_module_reaches_into_rnn_and_rnn_stands_without_the_vocoder():
    for path in MODULES:
        for node in ast.walk(_tree(path)):
            if isinstance(node, ast.ImportFrom) and node.module is not None and node.module.split(".")[-1] == "rnn":
                private = [a.name for a in node.names if a.name.startswith("_")]
                assert not private, (os.path.basename(path), private)
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "rnn":
                assert not node.attr.startswith("_"), (os.path.basename(path), node.attr)
    for node in ast.walk(_tree(os.path.join(PKG, "rnn.py"))):
        if isinstance(node, ast.ImportFrom):
            assert (node.module or "").split(".")[-1] != "vocoder" and all(a.name != "vocoder" for a in node.names)
        if isinstance(node, ast.Import):
            assert all(not a.name.endswith("vocoder") for a in node.names)


def test_both_eval_packs_live_in_the_one_cache(monkeypatch):
    """Vocoder._pack and rnn.pack_of on CPU-constructed modules, up to the cache call (building a pack is the first device use; the RNN
    models' own _pack refuses a CPU model before it gets to rnn.pack_of)."""
    from unast_amd import contract, rnn
    from unast_amd.network import TextRNN, SpeechRNN, Vocoder
    seen = []

    def counting(m, slot, tensors, build):
        assert callable(build) and all(torch.is_tensor(t) for t in tensors)
        seen.append((m, slot, len(tensors)))
        return "pack"
    monkeypatch.setattr(contract, "cached_operands", counting)
    voc = Vocoder(80, 256, 2048)
    tm, sm = TextRNN(rnn_weights.rnn_args("luong")), SpeechRNN(rnn_weights.rnn_args("lsa"))
    assert voc._pack() == "pack" and rnn.pack_of(tm, "text") == "pack" and rnn.pack_of(sm, "speech") == "pack"
    want = [(m, slot, len(list(m.parameters())) + len(list(m.buffers()))) for m, slot in ((voc, "_vocoder_pack"), (tm, "_rnn_pack"), (sm, "_rnn_pack"))]
    assert [(id(m), s, n) for m, s, n in seen] == [(id(m), s, n) for m, s, n in want]


def test_cached_operands_follows_version_counters():
    from unast_amd import contract
    m = torch.nn.Linear(3, 2)
    built = []
    build = lambda: built.append(1) or len(built)                                   # noqa: E731
    tensors = list(m.parameters())
    assert contract.cached_operands(m, "_slot", tensors, build) == 1 and contract.cached_operands(m, "_slot", tensors, build) == 1
    with torch.no_grad():
        m.bias.add_(1.0)
    assert contract.cached_operands(m, "_slot", tensors, build) == 2
    m.__dict__.pop("_slot")
    assert contract.cached_operands(m, "_slot", tensors, build) == 3 and "_slot" not in dict(m.named_parameters())


@pytest.fixture
def launches(monkeypatch):
    """Stand-ins for the four entry points the forward forms launch: they record their names and do nothing."""
    from unast_amd import ops
    calls = []
    for name in ("split_parts", "gemm", "conv_taps_fwd", "leaky_dropout"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    return calls


def _bad(good):
    """`good` with one row more, in float64, and on another device."""
    return [torch.empty(good.shape[0] + 1, *good.shape[1:]), torch.empty(good.shape, dtype=torch.float64), torch.empty(good.shape, device="meta")]


def test_linear_rows_refuses_wrong_out_and_work_before_any_launch(launches):
    from unast_amd import contract
    M, K, N, ld = 6, 8, 5, 8
    x, Wp, b = torch.zeros(M, K), (torch.zeros(N, K), torch.zeros(N, K)), torch.zeros(N)
    out = torch.zeros(M, ld)
    work = (torch.zeros(M, K), torch.zeros(M, K), torch.zeros(M, ld), torch.zeros(M, ld))
    for bad in _bad(out) + [torch.zeros(M, N - 1), torch.zeros(M, 2 * ld)[:, :ld], torch.zeros(M, 1, ld), [[0.0] * ld] * M]:
        with pytest.raises(ValueError, match="linear_rows: out"):
            contract.linear_rows(x, Wp, b, out=bad, work=work)
    for i in range(4):
        for bad in _bad(work[i]) + [torch.zeros(M, 2 * work[i].shape[1])[:, :work[i].shape[1]]]:
            with pytest.raises(ValueError, match="linear_rows: work"):
                contract.linear_rows(x, Wp, b, out=out, work=work[:i] + (bad,) + work[i + 1:])
    with pytest.raises(ValueError, match="linear_rows: work"):
        contract.linear_rows(x, Wp, b, out=out, work=work[:3])
    with pytest.raises(ValueError, match="linear_rows: work"):                       # partial sums at the pitch of `out`, not of W
        contract.linear_rows(x, Wp, b, out=out, work=work[:2] + (torch.zeros(M, N), torch.zeros(M, N)))
    assert launches == []
    y = contract.linear_rows(x, Wp, b, out=out, work=work)                           # the control: the same call with the right buffers launches
    assert launches == ["split_parts", "gemm", "gemm", "gemm"] and y.data_ptr() == out.data_ptr() and tuple(y.shape) == (M, N)


def test_conv_refuses_wrong_out_and_work_before_any_launch(launches):
    from unast_amd import contract
    B, T, Cin, Cout, taps = 2, 5, 8, 4, 3
    x, Wp, b = torch.zeros(B, T, Cin), (torch.zeros(Cout, taps, Cin), torch.zeros(Cout, taps, Cin)), torch.zeros(Cout)
    out = torch.zeros(B, T, Cout)
    work = (torch.zeros(B, T, Cin), torch.zeros(B, T, Cin), torch.zeros(B, T, Cout), torch.zeros(B, T, Cout))
    for bad in _bad(out) + [torch.zeros(B, T, Cout + 4), torch.zeros(B * T, Cout), "out"]:
        with pytest.raises(ValueError, match="conv: out"):
            contract.conv(x, Wp, b, 1, out=bad, work=work)
    for i in range(4):
        for bad in _bad(work[i]) + [torch.zeros(B, T, 2 * work[i].shape[2])[:, :, :work[i].shape[2]]]:
            with pytest.raises(ValueError, match="conv: work"):
                contract.conv(x, Wp, b, 1, out=out, work=work[:i] + (bad,) + work[i + 1:])
    with pytest.raises(ValueError, match="conv: work"):
        contract.conv(x, Wp, b, 1, work=work[1:])
    assert launches == []
    wide = torch.zeros(B, T, 3 * Cout)                                               # a column slice as `out` is what the tap kernels take
    assert contract.conv(x[:, :, :Cin], Wp, b, 1, out=wide[:, :, Cout:2 * Cout], work=work).data_ptr() == wide[:, :, Cout:].data_ptr()
    assert launches == ["split_parts", "conv_taps_fwd", "conv_taps_fwd", "conv_taps_fwd"]
