"""GPU parity of the single-position decoding kernels (csrc/decode.hip) against fp64 CPU math and against the general kernels
they stand in for (same dropout streams)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")


def relerr(a, b):
    return ((a.double().cpu() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("M,N,K", [(32, 768, 256), (3, 81, 256), (33, 46, 1024), (32, 256, 80), (1, 1024, 256), (70, 256, 1024), (32, 16, 4)])
def test_decode_linear_matches_fp64(M, N, K):
    from unast_amd import ops
    g = torch.Generator().manual_seed(M * 13 + N + K)
    x, W, b, R = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ldn = (N + 3) // 4 * 4
    y = torch.zeros(M, ldn, device=D)
    ops.decode_linear(x.to(D), W.to(D), b.to(D), y)
    assert relerr(y[:, :N], x.double() @ W.double().t() + b.double()) < 3e-5
    assert (y[:, N:] == 0).all(), "columns past N must not be written"
    y2 = torch.zeros(M, ldn, device=D)
    Rd = torch.zeros(M, ldn, device=D)
    Rd[:, :N] = R.to(D)
    ops.decode_linear(x.to(D), W.to(D), b.to(D), y2, act=1, R=Rd)
    assert relerr(y2[:, :N], torch.relu(x.double() @ W.double().t() + b.double()) + R.double()) < 3e-5
    y3 = torch.zeros(M, ldn, device=D)
    ops.decode_linear(x.to(D), W.to(D), None, y3)
    assert relerr(y3[:, :N], x.double() @ W.double().t()) < 3e-5


@pytest.mark.parametrize("M,N,K", [(32, 1024, 256), (5, 256, 256), (40, 768, 128)])
def test_decode_linear_fused_layernorm(M, N, K):
    from unast_amd import ops
    g = torch.Generator().manual_seed(M + N)
    z = torch.randn(M, K, generator=g) * 3 + 1
    gam, bet = torch.rand(K, generator=g) + .5, torch.randn(K, generator=g)
    W, b = torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    xn_ref = torch.nn.functional.layer_norm(z.double(), (K,), gam.double(), bet.double(), 1e-5)
    y = torch.zeros(M, N, device=D)
    xn = torch.zeros(M, K, device=D)
    ops.decode_linear(z.to(D), W.to(D), b.to(D), y, act=1, ln=(gam.to(D), bet.to(D)), xn_out=xn)
    assert relerr(xn, xn_ref) < 1e-5
    assert relerr(y, torch.relu(xn_ref @ W.double().t() + b.double())) < 3e-5


def test_decode_linear_appends_to_cache_at_device_position():
    from unast_amd import ops
    B, E, Tcap = 6, 256, 9
    g = torch.Generator().manual_seed(3)
    x, W, b = torch.randn(B, E, generator=g), torch.randn(3 * E, E, generator=g) * 0.1, torch.randn(3 * E, generator=g)
    ref = x.double() @ W.double().t() + b.double()
    cache = torch.zeros(B, Tcap, 2 * E, device=D)
    q = torch.zeros(B, E, device=D)
    pos = torch.tensor([4], dtype=torch.int64, device=D)
    ops.decode_linear(x.to(D), W.to(D), b.to(D), q, cache=cache, split_col=E, pos=pos)
    assert relerr(q, ref[:, :E]) < 3e-5
    assert relerr(cache[:, 4], ref[:, E:]) < 3e-5
    cache[:, 4] = 0
    assert (cache == 0).all(), "only row `pos` of every sequence may be written"


def test_decode_linear_dropout_uses_the_gemm_streams():
    """Same (seed, stream) => the mask of the general GEMM epilogue."""
    from unast_amd import ops
    M, N, K = 32, 256, 256
    g = torch.Generator().manual_seed(5)
    x, W, b = torch.randn(M, K, generator=g).to(D), (torch.randn(N, K, generator=g) * 0.1).to(D), torch.randn(N, generator=g).to(D)
    y1, y2 = torch.zeros(M, N, device=D), torch.zeros(M, N, device=D)
    ops.decode_linear(x, W, b, y1, drop_p=0.3, seed=11, stream_id=5)
    ops.linear_fwd(x, W, b, y2, drop_p=0.3, seed=11, stream_id=5)
    assert torch.equal(y1 == 0, y2 == 0)
    assert 0.2 < float((y1 == 0).float().mean()) < 0.4
    assert relerr(y1, y2.cpu()) < 3e-5


@pytest.mark.parametrize("B,H,Tcap,drop", [(32, 4, 800, 0.0), (3, 4, 37, 0.0), (5, 2, 300, 0.25)])
def test_decode_attn(B, H, Tcap, drop):
    from unast_amd import ops
    E = 64 * H
    g = torch.Generator().manual_seed(B + Tcap)
    q = torch.randn(B, E, generator=g)
    kv = torch.randn(B, Tcap, 2 * E, generator=g)
    lens = torch.randint(1, Tcap + 1, (B,), generator=g, dtype=torch.int32)
    lens[0] = Tcap
    lens[-1] = 1
    kvd = kv.to(D).view(B * Tcap, 2 * E)
    O = torch.zeros(B, E, device=D)
    ops.decode_attn(q.to(D), kvd[:, :E], kvd[:, E:], Tcap, O, H, lens=lens.to(D), drop_p=drop, seed=9, stream_id=2)
    # the general attention kernel with one query per sequence draws the same mask
    O2 = torch.zeros(B, E, device=D)
    lse = torch.zeros(B, H, 1, device=D)
    ops.attn_fwd(q.to(D), kvd[:, :E], kvd[:, E:], O2, lse, lens.to(D), B, H, 1, Tcap, False, drop_p=drop, seed=9, stream_id=2)
    assert relerr(O, O2.cpu()) < 2e-5
    if drop == 0.0:
        ref = torch.zeros(B, E, dtype=torch.float64)
        for b in range(B):
            n = int(lens[b])
            for h in range(H):
                qq = q[b, 64 * h:64 * h + 64].double()
                kk = kv[b, :n, 64 * h:64 * h + 64].double()
                vv = kv[b, :n, E + 64 * h:E + 64 * h + 64].double()
                ref[b, 64 * h:64 * h + 64] = torch.softmax(kk @ qq * 0.125, 0) @ vv
        assert relerr(O, ref) < 1e-5
    # valid length from the device-resident position and stop lengths: min(stop + 1, pos + 1)
    pos = torch.tensor([min(20, Tcap - 1)], dtype=torch.int64, device=D)
    stop = torch.full((B,), Tcap, dtype=torch.int64)
    stop[-1] = 3
    O3, O4 = torch.zeros(B, E, device=D), torch.zeros(B, E, device=D)
    ops.decode_attn(q.to(D), kvd[:, :E], kvd[:, E:], Tcap, O3, H, stop_lens=stop.to(D), pos=pos)
    ops.decode_attn(q.to(D), kvd[:, :E], kvd[:, E:], Tcap, O4, H, lens=torch.minimum(stop + 1, pos.cpu() + 1).to(torch.int32).to(D))
    assert torch.equal(O3, O4)


@pytest.mark.parametrize("drop", [0.0, 0.2])
def test_decode_linear_row_producers_match_the_standalone_kernels(drop):
    """Embedding + positional encoding, positional encoding alone and LayerNorm + dropout produced inside the contraction give
    what embed_fwd / posenc_fwd / layernorm_fwd / leaky_dropout followed by the plain contraction give (same dropout streams)."""
    import math
    from unast_amd import ops
    B, E, N, T, V = 7, 256, 96, 12, 46
    g = torch.Generator().manual_seed(21)
    tokens = torch.randint(0, V, (B, T), generator=g).to(D)
    emb, pe = torch.randn(V, E, generator=g).to(D), torch.randn(40, E, generator=g).to(D)
    W, b = (torch.randn(N, E, generator=g) * 0.1).to(D), torch.randn(N, generator=g).to(D)
    pos = torch.tensor([5], dtype=torch.int64, device=D)
    sc = math.sqrt(E)
    # embedding + positional encoding
    y, xn = torch.zeros(B, N, device=D), torch.zeros(B, E, device=D)
    ops.decode_linear(None, W, b, y, embed=(tokens, emb, pe, sc, (drop, 3), (drop, 4)), xn_out=xn, seed=17, pos=pos)
    x0, x1, y_ref = torch.zeros(B, E, device=D), torch.zeros(B, E, device=D), torch.zeros(B, N, device=D)
    ops.embed_fwd(tokens[:, 5].contiguous(), emb, x0, 1, drop_p=drop, seed=17, stream_id=3)
    ops.posenc_fwd(x0, pe[5:6], x1, 1, sc, drop_p=drop, seed=17, stream_id=4)
    ops.decode_linear(x1, W, b, y_ref)
    assert relerr(xn, x1.cpu()) < 1e-6 and relerr(y, y_ref.cpu()) < 1e-5
    # positional encoding of given rows, rows taken from a [B, T, K] buffer at the position
    frames = torch.randn(B, T, E, generator=g).to(D)
    y2, xn2 = torch.zeros(B, N, device=D), torch.zeros(B, E, device=D)
    ops.decode_linear(frames[:, 5].contiguous(), W, b, y2, posenc=(pe, sc, (drop, 6)), xn_out=xn2, seed=17, pos=pos)
    ops.posenc_fwd(frames[:, 5].contiguous(), pe[5:6], x1, 1, sc, drop_p=drop, seed=17, stream_id=6)
    ops.decode_linear(x1, W, b, y_ref)
    assert relerr(xn2, x1.cpu()) < 1e-6 and relerr(y2, y_ref.cpu()) < 1e-5
    y3 = torch.zeros(B, N, device=D)
    ops.decode_linear(None, W, b, y3, x_frames=frames, pos=pos)
    ops.decode_linear(frames[:, 5].contiguous(), W, b, y_ref)
    assert torch.equal(y3, y_ref)
    # LayerNorm + dropout
    z = (torch.randn(B, E, generator=g) * 2 + .5).to(D)
    gam, bet = (torch.rand(E, generator=g) + .5).to(D), torch.randn(E, generator=g).to(D)
    y4 = torch.zeros(B, N, device=D)
    ops.decode_linear(z, W, b, y4, ln=(gam, bet), ln_drop=(drop, 8), seed=17)
    xl, mean, rstd, xd = torch.zeros(B, E, device=D), torch.zeros(B, device=D), torch.zeros(B, device=D), torch.zeros(B, E, device=D)
    ops.layernorm_fwd(z, gam, bet, xl, mean, rstd)
    ops.leaky_dropout(xl, None, xd, 1.0, drop_p=drop, seed=17, stream_id=8)
    ops.decode_linear(xd, W, b, y_ref)
    assert relerr(y4, y_ref.cpu()) < 1e-5
    if drop > 0:
        assert torch.equal(y4 == 0, y_ref == 0) or relerr(y4, y_ref.cpu()) < 1e-5


# ---- decode_attn at the slot and round edges -----------------------------------------------------------------
EDGE_LENS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 520, 600, -3]


def decode_attn_ref(q, kv, n_keys, H, factor=None):
    """fp64 single-query attention of every (sequence, head) over its first n_keys[b] cached rows; factor [B, H, Tcap]: the dropout
    factor on the normalised probabilities.  No key: zeros."""
    B, E = q.shape
    ref = torch.zeros(B, E, dtype=torch.float64)
    for b in range(B):
        n = int(n_keys[b])
        for h in range(H if n > 0 else 0):
            c = slice(64 * h, 64 * h + 64)
            pr = torch.softmax(kv[b, :n, c].double() @ q[b, c].double() * 0.125, 0)
            if factor is not None:
                pr = pr * factor[b, h, :n]
            ref[b, c] = pr @ kv[b, :n, E + 64 * h:E + 64 * h + 64].double()
    return ref


def seq_relerr(a, b):
    """per sequence: max |a[b] - ref[b]| / max |ref[b]| (a length-1 sequence returns its V row, a long one an average many times smaller)"""
    b = b.double()
    return ((a.double().cpu() - b).abs().amax(1) / b.abs().amax(1).clamp_min(1e-30))


@pytest.fixture(scope="module")
def edge_qkv():
    H, Tcap, B = 2, 520, len(EDGE_LENS)
    g = torch.Generator().manual_seed(520)
    return H, Tcap, torch.randn(B, 64 * H, generator=g), torch.randn(B, Tcap, 128 * H, generator=g)


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_decode_attn_at_slot_and_round_edges(p, edge_qkv):
    """64 slots x 4 keys per round: lengths around one slot group (16), one pass of the slots (64), one round (256), two rounds (512), the
    cache size, past it and below zero (both clamped), and no key at all (exact zeros) -- against fp64, with dropout under the mirror's mask."""
    from tests import dropout_mirror as M
    from unast_amd import ops
    H, Tcap, q, kv = edge_qkv
    B, E = q.shape
    n_keys = torch.tensor(EDGE_LENS).clamp(0, Tcap)
    epoch = int(ops.rng_epoch_counter().item())          # mixed into every mask; 0 unless an earlier test left it advanced
    factor = torch.from_numpy(M.attn_keep(9, 2, B, H, 1, Tcap, p, epoch)[:, :, 0] * float(M.drop_scale(p))) if p > 0 else None
    ref = decode_attn_ref(q, kv, n_keys, H, factor)
    kvd = kv.to(D).view(B * Tcap, 2 * E)
    O = torch.full((B, E), float("nan"), device=D)
    ops.decode_attn(q.to(D), kvd[:, :E], kvd[:, E:], Tcap, O, H, lens=torch.tensor(EDGE_LENS, dtype=torch.int32, device=D), drop_p=p, seed=9, stream_id=2)
    assert bool(torch.isfinite(O).all())
    assert bool((O[n_keys == 0] == 0).all()), "a sequence without keys returns exact zeros"
    live = n_keys > 0
    err = seq_relerr(O[live], ref[live])
    print("decode_attn edges p=%.2f: worst per-sequence error %.1e at length %d (bound 1e-05)" % (p, float(err.max()), int(n_keys[live][err.argmax()])))
    assert relerr(O, ref) < 1e-5
    assert bool((err < 1e-5).all()), err.tolist()


@pytest.mark.parametrize("pos", [0, 300, 519])
def test_decode_attn_length_from_stop_lens_and_position(pos, edge_qkv):
    """n = min(stop_lens + 1, pos + 1) from the device-resident state, against fp64: the first position, the last row of the cache,
    a sequence stopped at 0, one stopped at this very position, one still running (stop_lens = max_len > pos), one stopped earlier."""
    from unast_amd import ops
    H, Tcap, q, kv = edge_qkv
    max_len = Tcap
    stop = torch.tensor([0, pos, max_len, min(7, pos), max(pos - 1, 0), max_len], dtype=torch.int64)
    B, E = stop.numel(), q.shape[1]
    q, kv = q[:B], kv[:B].contiguous()
    n_keys = torch.minimum(stop + 1, torch.tensor(pos + 1))
    ref = decode_attn_ref(q, kv, n_keys, H)
    kvd = kv.to(D).view(B * Tcap, 2 * E)
    O = torch.full((B, E), float("nan"), device=D)
    ops.decode_attn(q.to(D), kvd[:, :E], kvd[:, E:], Tcap, O, H, stop_lens=stop.to(D), pos=torch.tensor([pos], dtype=torch.int64, device=D))
    err = seq_relerr(O, ref)
    print("decode_attn stop_lens/pos=%d: worst per-sequence error %.1e (bound 1e-05)" % (pos, float(err.max())))
    assert bool((err < 1e-5).all()), err.tolist()


# ---- the end of a position: greedy choice / frame copy, stop rule, pos += 1, epoch += 1 --------------------------
MAX_LEN = 6


def _text_script(kind):
    """logits [MAX_LEN, B, ld] for MAX_LEN positions, V, eos"""
    g = torch.Generator().manual_seed(46)
    if kind == "many-rows":          # more rows than the workgroup's 256 threads; small integers: ties in most rows
        V, ld, eos, B = 5, 8, 2, 300
        x = torch.randint(-2, 3, (MAX_LEN, B, ld), generator=g).float()
        x[..., V:] = 9.0
        return x, V, eos
    V, ld, eos, B = 46, 48, 2, 12
    x = torch.randn(MAX_LEN, B, ld, generator=g)
    x[:, :, eos] = -9.0          # EOS only where scripted below
    x[..., V:] = 100.0           # the padding columns of the row pitch hold a larger value: never chosen
    x[:, 0, 5] = 7.0; x[:, 0, 9] = 7.0                      # row 0: a tie for the maximum, the first index wins
    x[2, 1, 1] = 7.0; x[2, 1, eos] = 7.0                    # row 1: EOS ties with an EARLIER column: no stop
    x[2, 2, eos] = 7.0; x[2, 2, 30] = 7.0                   # row 2: EOS ties with a LATER column: EOS, stop at 3
    x[0, 3, eos] = 7.0                                      # row 3: EOS at the first position
    x[1, 4, eos] = 7.0; x[3, 4, eos] = 7.0                  # row 4: EOS twice, the first one sticks
    x[MAX_LEN - 1, 5, eos] = 7.0                            # row 5: EOS exactly at i == max_len
    x[:, 6, :V] = -x[:, 6, :V].abs() - 1.0                  # row 6: all-negative rows
    x[:, 7, :V] = float("-inf"); x[:, 7, 17] = -3.0; x[4, 7, 17] = float("-inf")      # row 7: -inf entries, at position 5 nothing else
    x[3, 7, eos] = 0.0
    x[:, 8, :V] = 1.25                                      # row 8: all equal -> column 0
    x[:, 9, 0] = 50.0                                       # row 9: the maximum in column 0
    x[:, 10, V - 1] = 50.0                                  # row 10: ... and in the last column before the padding
    x[5, 11, eos] = 7.0; x[5, 11, 0] = 7.0                  # row 11: at i == max_len EOS ties with column 0: no stop
    return x, V, eos


@pytest.mark.parametrize("with_epoch", [True, False], ids=["epoch", "no-epoch"])
@pytest.mark.parametrize("kind", ["edges", "many-rows"])
def test_decode_end_text_position_by_position(kind, with_epoch):
    """unast_decode_end_text against the reference loop (src/network.py:466-473) in plain PyTorch, after every call and exact:
    tokens (the untouched columns too), stop_lens, pos and the RNG epoch."""
    from unast_amd import ops
    script, V, eos = _text_script(kind)
    B = script.shape[1]
    tokens = torch.full((B, MAX_LEN + 3), 77, dtype=torch.int64)
    tokens[:, 0] = 1
    stop_lens = torch.full((B,), MAX_LEN, dtype=torch.int64)
    tok_d, stop_d = tokens.to(D), stop_lens.to(D)
    pos_d = torch.zeros(1, dtype=torch.int64, device=D)
    epoch_d = torch.full((1,), 40, dtype=torch.int32, device=D) if with_epoch else None
    for i in range(1, MAX_LEN + 1):
        logits = script[i - 1]
        ops.decode_end_text(logits.to(D), V, tok_d, stop_d, MAX_LEN, eos, pos_d, epoch_d)
        choice = torch.argmax(logits[:, :V], dim=-1)
        tokens[:, i] = choice
        stop_mask = (choice == eos) & (stop_lens == MAX_LEN)
        stop_lens[stop_mask] = i
        assert torch.equal(tok_d.cpu(), tokens), (i, (tok_d.cpu() != tokens).nonzero().tolist()[:5])
        assert torch.equal(stop_d.cpu(), stop_lens), i
        assert int(pos_d) == i
        if with_epoch:
            assert int(epoch_d) == 40 + i
    if kind == "edges":          # the script did what it was written for
        assert tokens[0, 1:MAX_LEN + 1].tolist() == [5] * MAX_LEN and tokens[1, 3] == 1 and tokens[7, 5] == 0
        assert stop_lens.tolist() == [6, 6, 3, 1, 2, 6, 6, 4, 6, 6, 6, 6]
        assert tokens[5, MAX_LEN] == eos and tokens[11, MAX_LEN] == 0
    else:
        assert len(set(stop_lens.tolist())) == MAX_LEN


STOP_X = [0.0, -0.0, -1e-9, 1e-9, -1e-3, 30.0, -30.0]


def _speech_script(kind):
    """head rows [MAX_LEN, B, ld] = [frame | stop logit | padding], M"""
    g = torch.Generator().manual_seed(80)
    if kind == "many-rows":
        M, ld, B = 4, 8, 300
        x = torch.randn(MAX_LEN, B, ld, generator=g)
        return x, M
    M, ld = 80, 84
    B = len(STOP_X) + 3
    x = torch.randn(MAX_LEN, B, ld, generator=g)
    x[:, :, M] = -5.0                                       # no stop except where scripted
    x[:, :, M + 1:] = 40.0                                  # the padding of the row pitch is not a stop logit
    for b, v in enumerate(STOP_X):                          # rows 0-6: one value of the stop logit each, at position b % MAX_LEN + 1
        x[b % MAX_LEN, b, M] = v
    x[MAX_LEN - 1, 7, M] = 3.0                              # row 7: the stop exactly at i == max_len
    x[1, 8, M] = 2.0; x[3, 8, M] = 2.0                      # row 8: a second stop is ignored
    return x, M                                             # row 9: never stops


@pytest.mark.parametrize("with_epoch", [True, False], ids=["epoch", "no-epoch"])
@pytest.mark.parametrize("kind", ["edges", "many-rows"])
def test_decode_end_speech_position_by_position(kind, with_epoch):
    """unast_decode_end_speech against the reference loop (src/network.py:232-243): the frame copied bit for bit to outputs[:, pos + 1],
    the raw logit to stops[:, pos + 1], the stop rule sigmoid(x) >= .5 as torch evaluates it in fp32 on the CPU (exactly 0.5 at -1e-9:
    a stop, where real arithmetic says none), the first stop sticks; everything else untouched."""
    from unast_amd import ops
    script, M = _speech_script(kind)
    B = script.shape[1]
    outputs = torch.full((B, MAX_LEN + 1, M), 0.5)
    stops = torch.full((B, MAX_LEN + 1), 0.25)
    stop_lens = torch.full((B,), MAX_LEN, dtype=torch.int64)
    out_d, stops_d, stop_d = outputs.to(D), stops.to(D), stop_lens.to(D)
    pos_d = torch.zeros(1, dtype=torch.int64, device=D)
    epoch_d = torch.full((1,), 7, dtype=torch.int32, device=D) if with_epoch else None
    for i in range(1, MAX_LEN + 1):
        head = script[i - 1]
        ops.decode_end_speech(head.to(D), M, out_d, stops_d, stop_d, MAX_LEN, pos_d, epoch_d)
        outputs[:, i] = head[:, :M]
        stops[:, i] = head[:, M]
        stop_mask = (torch.sigmoid(head[:, M]) >= .5) & (stop_lens == MAX_LEN)
        stop_lens[stop_mask] = i
        assert torch.equal(out_d.cpu().view(torch.int32), outputs.view(torch.int32)), i
        assert torch.equal(stops_d.cpu().view(torch.int32), stops.view(torch.int32)), i
        assert torch.equal(stop_d.cpu(), stop_lens), (i, stop_d.cpu().tolist(), stop_lens.tolist())
        assert int(pos_d) == i
        if with_epoch:
            assert int(epoch_d) == 7 + i
    if kind == "edges":
        # torch's fp32 sigmoid: 0.5 exactly at 0, -0, -1e-9 and 1e-9 (a stop), below at -1e-3 and -30, above at 30
        assert stop_lens.tolist() == [1, 2, 3, 4, 6, 6, 6, 6, 2, 6]
        assert float(torch.sigmoid(torch.tensor(-1e-9))) == 0.5
    else:
        assert len(set(stop_lens.tolist())) == MAX_LEN


@pytest.mark.parametrize("Dm", [1, 80, 3])
def test_mask_by_len(Dm):
    """x[b, t] = 0 for t >= lens[b], exact: lengths 0, T and past T, a length that only an int64 holds (2^32 + 1 is 1 in 32 bits);
    the [B, T] stop tensor (D = 1), the frame tensor, an odd width; more than one workgroup."""
    from unast_amd import ops
    B, T = 6, 70
    g = torch.Generator().manual_seed(Dm)
    x = torch.randn(B, T, Dm, generator=g)
    lens = torch.tensor([0, T, T + 3, 33, 1, 2 ** 32 + 1], dtype=torch.int64)
    xd = x.to(D)
    ops.mask_by_len(xd if Dm > 1 else xd.view(B, T), lens.to(D))
    ref = x * (torch.arange(T)[None, :] < lens[:, None])[..., None]
    assert torch.equal(xd.cpu(), ref)
    assert bool((xd[0] == 0).all()) and torch.equal(xd[1].cpu(), x[1]) and torch.equal(xd[5].cpu(), x[5])


def test_argmax_rows():
    """Exact against torch.argmax (the first maximum): ties, a row of equal values, -inf entries and a row of nothing else, a row pitch
    wider than the row with larger values in the padding, 257 rows (two workgroups)."""
    from unast_amd import ops
    rows, cols, ld = 257, 46, 48
    g = torch.Generator().manual_seed(257)
    x = torch.randint(-3, 4, (rows, ld), generator=g).float()          # seven values over 46 columns: every row has ties
    x[:, cols:] = 99.0
    x[1, :cols] = 2.0
    x[2, :cols] = float("-inf"); x[2, 40] = -1e30; x[2, 44] = -1e30
    x[3, :cols] = float("-inf")
    x[4, :cols] = -5.0; x[4, cols - 1] = -4.0
    x[256, :cols] = -5.0; x[256, 0] = float("-inf"); x[256, 7] = 1.0; x[256, 9] = 1.0
    out = torch.full((rows,), -1, dtype=torch.int64, device=D)
    ops.argmax_rows(x.to(D), cols, out)
    ref = torch.argmax(x[:, :cols], dim=-1)
    assert torch.equal(out.cpu(), ref)
    assert ref[1] == 0 and ref[2] == 40 and ref[3] == 0 and ref[4] == cols - 1 and ref[256] == 7
