"""What the evaluation of the RNN family rests on, checked without a GPU: the C ABI header, unast_amd.ops and the documents agree on the new
entry points; csrc/metrics.hip keeps the package's kernel constraints; the reference fixtures (tests/golden/rnn_eval_{luong,lsa}.npz) hold the
decisions and margins the GPU test relies on; and compute_per_device and the entry points of unast_amd.eval_rnn refuse to run without a GPU."""
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rnn_eval_fixture as EF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_ops_and_documents_agree():
    from unast_amd import ops
    from unast_amd._lib import parse_header
    protos = parse_header()
    want = {"unast_edit_distance": 14, "unast_edit_distance_ws_bytes": 3, "unast_edit_distance_limits": 1}
    assert {k: len(protos[k][1]) for k in want} == want
    assert hasattr(ops, "edit_distance") and hasattr(ops, "edit_distance_limits")
    n = len(protos)
    for doc, pat in (("README.md", r"the C ABI \((\d+) entry points\)"), ("INTEGRATION.md", r"for every entry point \((\d+)\)")):
        m = re.search(pat, open(os.path.join(ROOT, doc)).read())
        assert m and int(m.group(1)) == n, (doc, m and m.group(1), n)
    src = open(os.path.join(ROOT, "unast_amd", "csrc", "metrics.hip")).read()
    for k in want:
        assert re.search(r'extern "C" \w+ %s\(' % k, src), k
    assert "atomic" not in src.replace("No atomics", "").replace("no atomics", "") and "cooperative" not in src.lower().replace("no cooperative launch", "")
    threads, chunk = (int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) for name in ("ED_THREADS", "ED_CHUNK"))
    assert (threads, chunk) == (ops.EDIT_THREADS, ops.EDIT_CHUNK) and ops.EDIT_MAX_COLS == threads * chunk == 65536


def test_nothing_runs_without_a_gpu():
    from unast_amd import eval_rnn, ops, utils
    from unast_amd.network import SpeechRNN, TextRNN, UNAST
    from tests import rnn_weights
    ids, lens = torch.tensor([[3, 4, 2]]), torch.tensor([3])
    with pytest.raises(TypeError, match="CUDA"):
        utils.compute_per_device(ids, ids, lens, lens)
    with pytest.raises(TypeError, match="CUDA"):
        ops.edit_distance(ids, lens.int(), ids, lens.int())
    model = UNAST(TextRNN(rnn_weights.rnn_args("luong")), SpeechRNN(rnn_weights.rnn_args("luong")))
    args = SimpleNamespace(use_discriminator=False)
    batch = (ids, torch.zeros(1, 4, 80), lens, torch.tensor([4]))
    for fn in (eval_rnn.autoencoder_losses, eval_rnn.supervised_losses, eval_rnn.crossmodel_losses):
        with pytest.raises(RuntimeError, match="GPU only|no CPU path|CUDA"):
            fn(model, batch, args)
    with pytest.raises(RuntimeError, match="GPU only|no CPU path|CUDA"):
        eval_rnn.evaluate(model, [batch], 0, args)
    with pytest.raises(ValueError, match="no discriminator"):
        eval_rnn.discriminator_eval(model, batch, SimpleNamespace(use_discriminator=True))
    with pytest.raises(TypeError, match="UNAST"):
        eval_rnn.autoencoder_losses(torch.nn.Linear(2, 2), batch, args)
    assert model.training, "a refused call leaves the model's mode alone"


@pytest.mark.parametrize("attn", EF.ATTNS)
def test_fixtures_hold_what_the_gpu_test_relies_on(attn):
    fx = EF.fixture(attn)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "rnn_eval_%s.npz" % attn)) <= 900000
    for case in EF.CASES:
        st = EF.setup(attn, case)
        margins = fx["%s/margins" % case]
        print(attn, case, "margins", margins, "asr lens", fx["%s/asr/lens" % case], "cm lens", fx["%s/cm/text_lens" % case], fx["%s/cm/speech_lens" % case],
              "tts lens", fx["%s/tts/stop_lens" % case])
        assert margins.min() >= 1e-2
        for k in EF.KEYS_D:
            assert np.isfinite(fx["%s/loss/%s" % (case, k)]) and fx["e32/%s/loss/%s" % (case, k)] <= EF.LOSS_TOL * max(1.0, abs(float(fx["%s/loss/%s" % (case, k)])))
        tok, lens = fx["%s/cm/tokens" % case], fx["%s/cm/text_lens" % case]
        live = np.arange(tok.shape[1])[None, :] < lens[:, None]
        assert not ((tok == 0) & live).any() and tok.shape[1] == lens.max()
        content = json.loads(str(fx["%s/json" % case]))
        text, _, tl, _ = EF.batch(attn, case)
        for b in range(st["B"]):
            assert content["utt%d" % b]["gt"] == text[b, :tl[b]].tolist()
            assert content["utt%d" % b]["pred"] == fx["%s/asr/tokens" % case][b, :fx["%s/asr/lens" % case][b]].tolist()
        if case == "b":        # one sequence of each generation never stops
            assert st["max_text"] in lens.tolist() and st["max_speech"] in fx["%s/cm/speech_lens" % case].tolist()


# ---- the fp64 mirror (tests/rnn_eval_mirror.py) -------------------------------------------------------------------------------------------------------------
def _mirror(attn, case, **kw):
    from tests import rnn_eval_mirror as EM
    from tests import rnn_step_fixture as SF
    st = EF.setup(attn, case)
    return EM.evaluate_batch(EF.state_dict(attn, case), attn, SF.args_of(attn, None), EF.batch(attn, case), st["max_text"], st["max_speech"], **kw)


@pytest.mark.parametrize("case", EF.CASES)
@pytest.mark.parametrize("attn", EF.ATTNS)
def test_mirror_reproduces_the_reference_fixtures(attn, case):
    fx, r = EF.fixture(attn), _mirror(attn, case)
    assert torch.equal(r["asr"][0], torch.from_numpy(fx["%s/asr/tokens" % case])) and r["asr"][1].tolist() == fx["%s/asr/lens" % case].tolist()
    assert torch.equal(r["cm_text"][0], torch.from_numpy(fx["%s/cm/tokens" % case])) and r["cm_text"][1].tolist() == fx["%s/cm/text_lens" % case].tolist()
    assert r["cm_speech"][3].tolist() == fx["%s/cm/speech_lens" % case].tolist() == fx["%s/tts/stop_lens" % case].tolist()
    worst = 0.0
    for k in EF.KEYS_D:
        want, got = float(fx["%s/loss/%s" % (case, k)]), r["losses"][k]
        worst = max(worst, abs(got - want) / max(1.0, abs(want)))
        assert abs(got - want) <= EF.LOSS_TOL * max(1.0, abs(want)), (k, got, want)
    post, stop = (np.abs(r["cm_speech"][i].numpy() - fx["%s/cm/%s" % (case, n)]).max() for i, n in ((1, "post"), (2, "stop")))
    print("%s %s: mirror vs the reference's fp64 run: losses %.2e relative, generated frames %.2e, stop logits %.2e" % (attn, case, worst, post, stop))
    assert post <= 1e-9 and stop <= 1e-9
    d_score = float(((torch.sigmoid(r["d_out"]).round() == r["d_target"].round()).sum()).item()) / EF.setup(attn, case)["B"] / 2
    assert d_score == float(fx["%s/d_score" % case])


def _noise(attn, case, seed=77):
    from tests import dropout_mirror as DM
    st = EF.setup(attn, case)
    B, T, Tm = st["B"], st["T_text"], st["T_mel"]
    return dict(text=torch.from_numpy(DM.row_keep(seed, 2, B * T, 0.3)).view(B, T), speech=torch.from_numpy(DM.row_keep(seed + 1, 2, B * Tm, 0.3)).view(B, Tm))


@pytest.mark.parametrize("fault", ["batch_stats", "dropout_on", "mask_after_prenet", "cm_disc_target_lens"])
@pytest.mark.parametrize("attn", EF.ATTNS)
def test_planted_faults_move_a_loss_by_100_times_the_gpu_bound(attn, fault):
    """Case a with the row masks on (p = 0.3, both encoders): each planted fault moves some loss by at least 100 x LOSS_TOL x max(1, |ref|), the
    bound tests/test_gpu_rnn_eval.py holds the losses to."""
    noise = _noise(attn, "a")
    assert not noise["text"].all() and not noise["speech"].all()
    only = ("cm",) if fault == "cm_disc_target_lens" else (("ae",) if fault == "mask_after_prenet" else None)
    ref = _mirror(attn, "a", noise=noise, only=only)["losses"]
    got = _mirror(attn, "a", noise=noise, only=only, fault=fault)["losses"]
    moved = {k: abs(got[k] - ref[k]) / (EF.LOSS_TOL * max(1.0, abs(ref[k]))) for k in ref}
    print(attn, fault, "moves, in units of the GPU bound:", {k: round(v, 1) for k, v in moved.items()})
    assert max(moved.values()) >= 100.0
