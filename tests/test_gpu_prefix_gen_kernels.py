"""The kernels of train-mode generation (csrc/prefix_gen.hip: unast_prefix_gen_conv, unast_prefix_gen_finish, unast_prefix_gen_act_drop,
unast_prefix_gen_end_text, unast_prefix_gen_end_speech) against fp64 torch on random tokens and weights.

One prefix is a [B, L, 256] batch: three launches of the conv kernel and one of the finish kernel are TextPrenet in train mode on it, keeping each
sequence's last row.  Shapes (B, L): (2,1) two identical rows, zero variance; (2,2), (3,3), (3,6) prefixes shorter than the three convs' receptive
field; (5,3) and (4,4) 15 and 16 rows, the MFMA tile's edge; (3,11) 33 rows, (7,40) and (2,130) several workgroups with sequence boundaries inside a
tile and on its edges.  Every buffer row past B*L holds NaN, the token buffer from L - 1 on points at a NaN row of the table, and the prefixes hold
PAD ids.  Bounds are tests/test_gpu_text_prefix_kernels.py's for the same quantities: forward 1e-3 x max|ref|, the running statistics 2e-5 against
the sequential fp32 torch update, num_batches_tracked exactly."""
import functools

import numpy as np
import pytest
import torch

from tests import dropout_mirror as DM

pytestmark = pytest.mark.gpu

C, V = 256, 46
SHAPES = [(2, 1), (2, 2), (3, 3), (3, 6), (5, 3), (4, 4), (3, 11), (7, 40), (2, 130)]
PS = [0.0, 0.5]
EPSS = [1e-5, 0.1]
SEED, ROW0, MOM = 31, 1000, 0.1
S_EMB, S_PRE = 21, 22
FWD_TOL, RUN_TOL = 1e-3, 2e-5
SOS = 1


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _weights():
    r = np.random.RandomState(5)
    E = torch.from_numpy(r.standard_normal((V, C))).float()                                            # row 0 (PAD) is not zero: nothing may lean on it
    Ws = [torch.from_numpy(r.standard_normal((C, C, 5)) / np.sqrt(5 * C) * 1.5).float() for _ in range(3)]
    bs = [torch.from_numpy(r.standard_normal(C) * 0.2).float() for _ in range(3)]
    gs = [torch.from_numpy(r.uniform(0.5, 1.5, C)).float() for _ in range(3)]
    be = [torch.from_numpy(r.standard_normal(C) * 0.3).float() for _ in range(3)]
    rm0 = [torch.from_numpy(r.standard_normal(C)).float() for _ in range(3)]
    rv0 = [torch.from_numpy(r.uniform(0.5, 2.0, C)).float() for _ in range(3)]
    return E, Ws, bs, gs, be, rm0, rv0


def _epoch():
    """The RNG epoch the kernels mix into their masks right now (0 unless an earlier captured step left its step number in the device counter)."""
    from unast_amd import ops
    return int(ops.rng_epoch_counter())


@functools.lru_cache(maxsize=None)
def _case(B, L, p, eps, epoch=0):
    """Tokens and the fp64 reference of one (B, L, p, eps) under the masks of one RNG epoch, computed once and left unchanged."""
    E, Ws, bs, gs, be, rm0, rv0 = _weights()
    r = np.random.RandomState(100 * B + L)
    toks = torch.from_numpy(r.randint(0, V, size=(B, max(L - 1, 1))).astype(np.int64))
    if L > 2:
        toks[0, 0] = 0                                                                                 # PAD ids inside the prefix
        toks[B - 1, L - 2] = 0
    ids = torch.cat([torch.full((B, 1), SOS, dtype=torch.int64), toks[:, :L - 1]], 1)                 # [B, L]
    N = B * L
    rows = ROW0 + np.arange(N)
    f = lambda stream: torch.from_numpy(DM.drop_factor(SEED, stream, rows, C, p, epoch)).view(B, L, C) if p > 0 else 1.0   # noqa: E731
    x = E.double()[ids] * f(S_EMB)
    zs, rms, rvs = [], [], []
    for i in range(3):
        z = torch.nn.functional.conv1d(x.transpose(1, 2), Ws[i].double(), bs[i].double(), padding=2).transpose(1, 2)        # every sequence on its own
        flat = z.reshape(N, C)
        mean, var = flat.mean(0), flat.var(0, unbiased=False)
        x = torch.relu((z - mean) / torch.sqrt(var + eps) * gs[i].double() + be[i].double()) * f(S_PRE + i)
        zs.append(flat)
        # the running statistics as torch keeps them: fp32, one momentum update from fp32 statistics
        rms.append((1 - MOM) * rm0[i] + MOM * mean.float())
        rvs.append((1 - MOM) * rv0[i] + MOM * (var * N / (N - 1)).float())
    return dict(toks=toks, zs=zs, pre=x[:, -1], rm=rms, rv=rvs)


def _bns(eps):
    E, Ws, bs, gs, be, rm0, rv0 = _weights()
    out = []
    for i in range(3):
        bn = torch.nn.BatchNorm1d(C, eps=eps, momentum=MOM).to(_dev())
        with torch.no_grad():
            bn.weight.copy_(gs[i]), bn.bias.copy_(be[i]), bn.running_mean.copy_(rm0[i]), bn.running_var.copy_(rv0[i])
        out.append(bn)
    return out


def _run(B, L, p, eps, running=None):
    from unast_amd import ops
    E, Ws, bs, gs, be, rm0, rv0 = _weights()
    cs, dev = _case(B, L, p, eps, _epoch()), _dev()
    N = B * L
    nan = float("nan")
    emb = torch.cat([E, torch.full((1, C), nan)]).to(dev)                                              # row V: what a read past the prefix would fetch
    tokens = torch.full((B, L + 6), V, dtype=torch.int64)
    tokens[:, :L - 1] = cs["toks"][:, :L - 1]
    tokens = tokens.to(dev)
    tiles = ops.prefix_gen_tiles(B, L)
    assert tiles == (N + 31) // 32
    zs = [torch.full((N + 40, C), nan, device=dev) for _ in range(3)]
    part = torch.full((3, tiles, 2, C), nan, dtype=torch.float64, device=dev)
    bns = _bns(eps)
    pre = torch.full((B, C), 7.0, device=dev)
    for i in range(3):
        Wp = Ws[i].permute(0, 2, 1).contiguous().to(dev)
        if i == 0:
            ops.prefix_gen_conv(Wp, bs[i].to(dev), zs[0], part[0], B, L, tokens=tokens, emb=emb, sos=SOS, drop_p=p, seed=SEED, stream_id=S_EMB, row0=ROW0)
        else:
            bn = bns[i - 1]
            ops.prefix_gen_conv(Wp, bs[i].to(dev), zs[i], part[i], B, L, x=zs[i - 1], part_in=part[i - 1], bn=(bn.weight, bn.bias, bn.eps), drop_p=p,
                                seed=SEED, stream_id=S_PRE + i - 1, row0=ROW0)
    ops.prefix_gen_finish(zs[2], part, bns, pre, B, L, running=running, drop_p=p, seed=SEED, stream_id=S_PRE + 2, row0=ROW0)
    torch.cuda.synchronize()
    for z in zs:
        assert torch.isnan(z[N:]).all(), "rows past B*L must not be written"
    return dict(zs=[z[:N] for z in zs], pre=pre, part=part, rm=[bn.running_mean for bn in bns], rv=[bn.running_var for bn in bns],
                nbt=[int(bn.num_batches_tracked) for bn in bns])


def _close(name, got, ref, tol):
    got, ref = got.detach().cpu().double(), ref.double()
    assert torch.isfinite(got).all(), name
    err, mx = (got - ref).abs().max().item(), ref.abs().max().item()
    print("%-22s err %.3g = %.3g of max|ref|" % (name, err, err / mx))
    assert err <= tol * mx, (name, err, mx)


@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,L", SHAPES)
def test_single_prefix_prenet(B, L, p, eps):
    cs = _case(B, L, p, eps, _epoch())
    a = _run(B, L, p, eps)
    for i in range(3):
        _close("z%d" % (i + 1), a["zs"][i], cs["zs"][i], FWD_TOL)
        _close("running_mean%d" % (i + 1), a["rm"][i], cs["rm"][i], RUN_TOL)
        _close("running_var%d" % (i + 1), a["rv"][i], cs["rv"][i], RUN_TOL)
    _close("pre", a["pre"], cs["pre"], FWD_TOL)
    assert a["nbt"] == [1, 1, 1]
    b = _run(B, L, p, eps)
    for k in ("zs", "rm", "rv"):
        assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), "two runs must agree to the bit: " + k
    assert torch.equal(a["pre"], b["pre"]) and torch.equal(a["part"], b["part"])


@pytest.mark.parametrize("B,L", [(2, 1), (3, 11)])
def test_running_predicate_off_leaves_the_statistics(B, L):
    E, Ws, bs, gs, be, rm0, rv0 = _weights()
    on = _run(B, L, 0.5, 1e-5, running=torch.ones((), dtype=torch.int32, device=_dev()))
    off = _run(B, L, 0.5, 1e-5, running=torch.zeros((), dtype=torch.int32, device=_dev()))
    assert on["nbt"] == [1, 1, 1] and off["nbt"] == [0, 0, 0]
    for i in range(3):
        assert torch.equal(off["rm"][i].cpu(), rm0[i]) and torch.equal(off["rv"][i].cpu(), rv0[i]), "bit-unchanged with the predicate off"
        assert not torch.equal(on["rm"][i].cpu(), rm0[i])
    assert torch.equal(on["pre"], off["pre"]), "the prenet's output does not depend on the predicate"


def test_zero_variance_prefix():
    """Position 0: B identical [SOS] rows.  x - mean is exactly zero at every stage with p = 0, so pre = relu(beta3) whatever eps."""
    E, Ws, bs, gs, be, rm0, rv0 = _weights()
    a = _run(2, 1, 0.0, 1e-5)
    assert torch.equal(a["zs"][0][0], a["zs"][0][1])
    assert (a["pre"].cpu() - torch.relu(be[2])[None, :]).abs().max().item() <= 1.5e-4                 # test_gpu_text_prefix_kernels.py's bound for this case


@pytest.mark.parametrize("p", PS)
def test_act_drop_rows(p):
    from unast_amd import ops
    dev, B = _dev(), 5
    x = torch.from_numpy(np.random.RandomState(2).standard_normal((B, 8, C))).float().to(dev)[:, 3]   # a row-strided view
    out = torch.empty(B, C, device=dev)
    row0 = 7 * B
    fa = torch.from_numpy(DM.drop_factor(SEED, 26, row0 + np.arange(B), C, p, _epoch())) if p > 0 else 1.0
    fb = torch.from_numpy(DM.drop_factor(SEED, 27, row0 + np.arange(B), C, 0.3 * (p > 0), _epoch()))
    for act, fn in ((ops.PGEN_NONE, lambda t: t), (ops.PGEN_TANH, torch.tanh), (ops.PGEN_RELU, torch.relu)):
        ops.prefix_gen_act_drop(x, out, act, drop_a=p, stream_a=26, drop_b=0.3 * (p > 0), stream_b=27, seed=SEED, row0=row0)
        _close("act %d" % act, out, fn(x.cpu().double()) * fa * fb, 1e-6)


def test_end_of_a_text_position():
    from unast_amd import ops
    dev, B, max_len, EOS = _dev(), 4, 6, 2
    logits = torch.full((B, 48), -1.0, device=dev)
    logits[0, 5] = logits[0, 9] = 3.0                                                                  # a tie: the first maximum
    logits[1, EOS] = 2.0
    logits[2, 0] = 1.0                                                                                 # PAD
    logits[3, 46] = 9.0                                                                                # a padding column of the head: not a candidate
    logits[3, 7] = 0.5
    tokens = torch.full((B, max_len), -5, dtype=torch.int64, device=dev)
    stop = torch.full((B,), max_len, dtype=torch.int64, device=dev)
    stop[2] = 1                                                                                        # stopped earlier: keeps its length
    run = torch.ones((), dtype=torch.int32, device=dev)
    ops.prefix_gen_end_text(logits, V, tokens, 3, stop, max_len, EOS, run)
    assert tokens[:, 3].tolist() == [5, EOS, 0, 7] and (tokens[:, :3] == -5).all() and (tokens[:, 4:] == -5).all()
    assert stop.tolist() == [max_len, 4, 1, max_len] and int(run) == 1
    logits[0, EOS] = logits[3, EOS] = 10.0
    ops.prefix_gen_end_text(logits, V, tokens, 4, stop, max_len, EOS, run)
    assert stop.tolist() == [5, 4, 1, 5] and int(run) == 0
    ops.prefix_gen_end_text(logits, V, tokens, 5, stop, max_len, EOS, run)                            # not running: nothing moves
    assert (tokens[:, 5] == -5).all() and stop.tolist() == [5, 4, 1, 5] and int(run) == 0


def test_end_of_a_speech_position():
    from unast_amd import ops
    dev, B, M, max_len = _dev(), 3, 80, 5
    head = torch.from_numpy(np.random.RandomState(3).standard_normal((B, 84))).float().to(dev)
    head[:, M] = torch.tensor([-0.1, 0.0, 2.0])                                                        # sigmoid(0) = .5 stops
    frames = torch.zeros(B, max_len + 1, M, device=dev)
    stops = torch.zeros(B, max_len, device=dev)
    stop = torch.full((B,), max_len, dtype=torch.int64, device=dev)
    run = torch.ones((), dtype=torch.int32, device=dev)
    ops.prefix_gen_end_speech(head, M, frames, stops, 1, stop, max_len, run)
    assert torch.equal(frames[:, 2], head[:, :M]) and frames[:, :2].abs().max().item() == 0 and frames[:, 3:].abs().max().item() == 0
    assert torch.equal(stops[:, 1], head[:, M]) and stop.tolist() == [max_len, 2, 2] and int(run) == 1
    head[0, M] = 0.3
    ops.prefix_gen_end_speech(head, M, frames, stops, 2, stop, max_len, run)
    assert stop.tolist() == [3, 2, 2] and int(run) == 0
    ops.prefix_gen_end_speech(head, M, frames, stops, 3, stop, max_len, run)
    assert frames[:, 4].abs().max().item() == 0 and stops[:, 3].abs().max().item() == 0 and stop.tolist() == [3, 2, 2]


def test_arguments_are_refused_before_a_launch():
    from unast_amd import ops
    dev = _dev()
    z, part = torch.empty(8, C, device=dev), torch.empty(1, 2, C, dtype=torch.float64, device=dev)
    Wp, b = torch.empty(C, 5, C, device=dev), torch.empty(C, device=dev)
    tok, emb = torch.zeros(1, 4, dtype=torch.int64, device=dev), torch.empty(V, C, device=dev)
    with pytest.raises(ValueError, match="2 <= B"):
        ops.prefix_gen_conv(Wp, b, z, part, 1, 4, tokens=tok, emb=emb, sos=SOS)
    with pytest.raises(ValueError, match=r"z must be contiguous \[>= B\*L"):
        ops.prefix_gen_conv(Wp, b, z, part, 2, 5, tokens=tok.expand(2, 4).contiguous(), emb=emb, sos=SOS)
    with pytest.raises(ValueError, match="give x, part_in and bn"):
        ops.prefix_gen_conv(Wp, b, z, part, 2, 4)
