"""acehip_lm_score_bf16 (csrc/lm_score.hip), HipCausalLM.score and the install_lm_score seam.

Kernel, exact: x and W hold {-1, 0, 1} with at most 256 non-zeros per W row, so every logit is an
integer of magnitude <= 256: exact in fp32 in any summation order and exact in bf16.  The counts
must then equal torch's integer computation, and lse / logprob are bounded against fp64 by
    (L + 8) * 2^-24 + |lse| * 2^-23
where L = 40 + ceil(ceil(V / 128) / 64) is the longest chain of fp32 additions that feeds one lse
(the kernel's header comment): a sum of positive terms over a chain of L additions is off by at
most L * 2^-24 relative, which is the absolute error of its log; the 8 covers the ulps of exp, of
the rescale and of log; |lse| * 2^-23 the final roundings.  (The kernel folds the per-tile sums in
fp64, so only the first 34 additions of the chain are fp32: the bound is not tightened for that.)  logprob = target logit (exact) - lse
has the same bound.

Kernel, random: Gaussian x and 0.05 * Gaussian W as test_gpu_lm_head.py; logprob against the fp64
log-softmax of bf16(x.float() @ W.float().T) with 2^-8 * max|logit| added to the bound above (one
bf16 rounding step of the target logit under another summation order).  Counts are asserted on the
rows where no other logit of the reference lies within that band of the target's.

Fixtures (tools/record_lm_score.py), through HipCausalLM.score: the RMS over positions of
(log-prob - fp32 fixture) is at most twice the manifest's ref_bf16_lp_rms (what the reference's own
bf16 model makes against its fp32 run; the rule of test_gpu_lm_decode.py); the ranks equal the fp32
ranks on every position the manifest marks clear; a scoring call between decode steps leaves the
generation's later logits bit-identical.

Measured on an MI355X.  Exact cases: lse error at most 2.0e-6 and logprob error at most 3.4e-6
against bounds of 4.6e-6 … 8.2e-6.  Random cases: logprob error 4.6e-7 / 1.7e-5 / 5.8e-6 against
1.5e-2 / 3.3e-2 / 4.8e-2, rows with no logit in the band 0.70 / 0.53 / 0.70.  Fixtures, log-prob RMS
against the fp32 run / bound: tiny 0.00420 / 0.00792, w06 0.04442 / 0.11729, w17 0.07747 / 0.15583;
means -5.03137 (fp32 run -5.03345), -3.50935 (-3.49792), -5.92272 (-5.93177)."""
import json
import math
import os

import pytest
import torch
from safetensors import safe_open

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NMAX = 70001
SENT_F, SENT_I = 1234.5, 777


def chain_len(V):
    """L of csrc/lm_score.hip's header comment."""
    return 40 + math.ceil(math.ceil(V / 128) / 64)


def lse_bound(V, lse_abs):
    return (chain_len(V) + 8) * 2.0 ** -24 + lse_abs * 2.0 ** -23


class Scored:
    def __init__(self, x, W, targets, T=None, V=None, K=None, ldx=None, ws_bytes=None, pad=5, ws_pad=256):
        from acehip import _ffi as ff
        dev = x.device
        T = x.shape[0] if T is None else T
        V = W.shape[0] if V is None else V
        K = x.shape[1] if K is None else K
        self.T = T
        n = max(T, 1) + pad
        self.lp = torch.full((n,), SENT_F, device=dev)
        self.lse = torch.full((n,), SENT_F, device=dev)
        self.ng = torch.full((n,), SENT_I, device=dev, dtype=torch.int32)
        self.ne = torch.full((n,), SENT_I, device=dev, dtype=torch.int32)
        need = int(ff.lib().acehip_lm_score_ws_bytes(max(T, 1), max(V, 1)))
        self.need = need
        self.ws = torch.full((need + ws_pad,), 0x5A, device=dev, dtype=torch.uint8)
        tg = targets.to(device=dev, dtype=torch.int32).contiguous()
        self.rc = ff.lib().acehip_lm_score_bf16(
            ff.ptr(x), x.stride(0) if ldx is None else ldx, ff.ptr(W), ff.ptr(tg), T, V, K, ff.ptr(self.lp),
            ff.ptr(self.lse), ff.ptr(self.ng), ff.ptr(self.ne), ff.ptr(self.ws),
            need if ws_bytes is None else ws_bytes, ff.stream_ptr())
        torch.cuda.synchronize()

    def untouched_outside(self):
        T = self.T
        return (bool((self.lp[T:] == SENT_F).all()) and bool((self.lse[T:] == SENT_F).all())
                and bool((self.ng[T:] == SENT_I).all()) and bool((self.ne[T:] == SENT_I).all())
                and bool((self.ws[self.need:] == 0x5A).all()))

    def untouched(self):
        return (bool((self.lp == SENT_F).all()) and bool((self.lse == SENT_F).all()) and bool((self.ng == SENT_I).all())
                and bool((self.ne == SENT_I).all()) and bool((self.ws == 0x5A).all()))


# ------------------------------------------------------------------ kernel, exact
@pytest.fixture(scope="module")
def int_weights(gpu_device):
    """Per K a [NMAX, K] table of {-1, 0, 1} with P(non-zero) = min(1, 128 / K): a row has
    128 non-zeros on average and (asserted) never more than 256."""
    out = {}
    for K in (256, 1024, 2048):
        g = torch.Generator(device=gpu_device).manual_seed(100 + K)
        nz = torch.rand(NMAX, K, device=gpu_device, generator=g) < min(1.0, 128.0 / K)
        sg = torch.randint(0, 2, (NMAX, K), device=gpu_device, generator=g) * 2 - 1
        W = (nz * sg).to(torch.bfloat16)
        assert int((W != 0).sum(1).max()) <= 256
        out[K] = W
    return out


def _special_targets(V):
    """Column 0, V - 1, one in the ragged last column tile, one in an interior tile."""
    last0 = (V - 1) // 128 * 128
    cols = [0, V - 1, min(V - 1, last0 + (V - last0) // 2), min(V - 1, 128 + 77 if V > 256 else 64)]
    return cols


@pytest.mark.parametrize("K", [256, 1024, 2048])
@pytest.mark.parametrize("V", [130, 4099, NMAX])
@pytest.mark.parametrize("T", [1, 37, 129])
def test_exact_counts_and_lse(gpu_device, int_weights, T, V, K):
    W = int_weights[K][:V].clone()
    cols = _special_targets(V)
    # ties at the target's value on both sides of the target's index: copies of the target's W row
    for c in cols:
        for d in (-1, 1, -129, 129, -(V // 2), V // 2):
            if 0 <= c + d < V and c + d not in cols:
                W[c + d] = W[c]
    g = torch.Generator().manual_seed(T * 7 + V + K)
    x = torch.randint(-1, 2, (T, K), generator=g).to(torch.bfloat16).to(gpu_device)
    rnd = torch.randint(0, V, (T,), generator=g)
    targets = torch.tensor([cols[r % 8] if r % 8 < 4 else int(rnd[r]) for r in range(T)])
    if T == 1:
        targets = torch.tensor([cols[(V + K) % 4]])
    s = Scored(x, W, targets)
    assert s.rc == 0
    logits = x.float() @ W.float().T                     # integers <= 256 in magnitude: exact in fp32
    assert float(logits.abs().max()) <= 256
    tg = targets.to(gpu_device)
    tl = logits.gather(1, tg[:, None])
    col = torch.arange(V, device=gpu_device)[None, :]
    ng = (logits > tl).sum(1)
    ne = ((logits == tl) & (col < tg[:, None])).sum(1)
    assert torch.equal(s.ng[:T].long(), ng), (s.ng[:T].tolist(), ng.tolist())
    assert torch.equal(s.ne[:T].long(), ne), (s.ne[:T].tolist(), ne.tolist())
    assert int(ne.max()) > 0 or T == 1                   # the planted ties are there
    lse = torch.logsumexp(logits.double(), dim=1)
    bound = lse_bound(V, lse.abs())
    e_lse = (s.lse[:T].double() - lse).abs()
    e_lp = (s.lp[:T].double() - (tl[:, 0].double() - lse)).abs()
    print(f"T{T} V{V} K{K}: lse err max {float(e_lse.max()):.3e}, logprob err max {float(e_lp.max()):.3e}, "
          f"bound min {float(bound.min()):.3e}")
    assert bool((e_lse <= bound).all()), (float(e_lse.max()), float(bound.min()))
    assert bool((e_lp <= bound).all()), (float(e_lp.max()), float(bound.min()))
    assert s.untouched_outside()
    again = Scored(x, W, targets)                        # same input, same bits
    assert again.rc == 0
    for a, b in ((s.lp, again.lp), (s.lse, again.lse)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(s.ng, again.ng) and torch.equal(s.ne, again.ne)


def test_row_stride_and_row_groups(gpu_device, int_weights):
    """ldx > K (rows of a wider buffer), and T = 1100: nine row tiles, so two row-tile groups."""
    K, V, T = 256, 515, 1100
    W = int_weights[K][:V].contiguous()
    g = torch.Generator().manual_seed(5)
    buf = torch.randint(-1, 2, (T, K + 64), generator=g).to(torch.bfloat16).to(gpu_device)
    x = buf[:, :K]
    targets = torch.randint(0, V, (T,), generator=g)
    s = Scored(x, W, targets)
    assert s.rc == 0
    logits = x.float() @ W.float().T
    tg = targets.to(gpu_device)
    tl = logits.gather(1, tg[:, None])
    col = torch.arange(V, device=gpu_device)[None, :]
    assert torch.equal(s.ng[:T].long(), (logits > tl).sum(1))
    assert torch.equal(s.ne[:T].long(), ((logits == tl) & (col < tg[:, None])).sum(1))
    lse = torch.logsumexp(logits.double(), dim=1)
    assert bool(((s.lse[:T].double() - lse).abs() <= lse_bound(V, lse.abs())).all())
    assert s.untouched_outside()


# ------------------------------------------------------------------ kernel, random
@pytest.mark.parametrize("T,V,K,seed", [(37, 4099, 256, 1), (129, NMAX, 1024, 2), (64, 4099, 2048, 3)])
def test_random_vs_fp64(gpu_device, T, V, K, seed):
    """Three quarters of the rows take the reference's 1st, 2nd or 3rd ranked token as target (the
    tail of a Gaussian row is sparse, so such a target has no neighbour within the band), one
    quarter a random token (which has hundreds).  The seeds are the first tried."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(V, K, generator=g) * 0.05).bfloat16().to(gpu_device)
    x = torch.randn(T, K, generator=g).bfloat16().to(gpu_device)
    ref = (x.float() @ W.float().T).bfloat16().float()
    top = ref.topk(3, dim=1).indices.cpu()
    rnd = torch.randint(0, V, (T,), generator=g)
    targets = torch.tensor([int(top[r, r % 3]) if r % 4 else int(rnd[r]) for r in range(T)])
    s = Scored(x, W, targets)
    assert s.rc == 0
    tg = targets.to(gpu_device)
    tl = ref.gather(1, tg[:, None])
    lse = torch.logsumexp(ref.double(), dim=1)
    band = 2.0 ** -8 * float(ref.abs().max())
    bound = lse_bound(V, lse.abs()) + band
    err = (s.lp[:T].double() - (tl[:, 0].double() - lse)).abs()
    print(f"T{T} V{V} K{K}: logprob err max {float(err.max()):.3e}, bound min {float(bound.min()):.3e}")
    assert bool((err <= bound).all()), (float(err.max()), float(bound.min()))
    col = torch.arange(V, device=gpu_device)[None, :]
    near = ((ref - tl).abs() <= band) & (col != tg[:, None])
    ok = ~near.any(1)
    share = float(ok.float().mean())
    print(f"  rows with no logit within the band of the target: {share:.2f}")
    assert share >= 0.5, share
    ng = (ref > tl).sum(1)
    ne = ((ref == tl) & (col < tg[:, None])).sum(1)
    assert torch.equal(s.ng[:T].long()[ok], ng[ok])
    assert torch.equal(s.ne[:T].long()[ok], ne[ok])
    assert s.untouched_outside()


# ------------------------------------------------------------------ arguments
def test_arguments(gpu_device, int_weights):
    from acehip import _ffi as ff
    K, V, T = 256, 515, 9
    W = int_weights[K][:V].contiguous()
    x = torch.ones(T, K, device=gpu_device, dtype=torch.bfloat16)
    xw = torch.ones(T, K + 4, device=gpu_device, dtype=torch.bfloat16)
    tg = torch.zeros(T, dtype=torch.int32)
    bad = [
        dict(T=0), dict(T=8193), dict(V=0), dict(V=(1 << 23) + 1), dict(K=200), dict(K=0),
        dict(ldx=K - 8), dict(ldx=K + 4), dict(ws_bytes=int(ff.lib().acehip_lm_score_ws_bytes(T, V)) - 1),
    ]
    for kw in bad:
        s = Scored(xw[:, :K] if kw.get("ldx") == K + 4 else x, W, tg, **kw)
        assert s.rc == -1, kw
        assert s.untouched(), kw
    # null pointers
    s = Scored(x, W, tg)
    lib, P = ff.lib(), ff.ptr
    dtg = tg.to(gpu_device)
    args = [P(x), K, P(W), P(dtg), T, V, K, P(s.lp), P(s.lse), P(s.ng), P(s.ne), P(s.ws), s.need, ff.stream_ptr()]
    before = [t.clone() for t in (s.lp, s.lse, s.ng, s.ne)]
    for i in (0, 2, 3, 7, 8, 9, 10, 11):
        a = list(args)
        a[i] = None
        assert lib.acehip_lm_score_bf16(*a) == -1, i
    torch.cuda.synchronize()
    for t, b in zip((s.lp, s.lse, s.ng, s.ne), before):
        assert torch.equal(t, b)


def test_target_out_of_range(gpu_device, int_weights):
    K, V, T = 256, 515, 40
    W = int_weights[K][:V].contiguous()
    g = torch.Generator().manual_seed(9)
    x = torch.randint(-1, 2, (T, K), generator=g).to(torch.bfloat16).to(gpu_device)
    good = torch.randint(0, V, (T,), generator=g)
    tg = good.clone()
    bad_rows = {3: -1, 17: V, 18: V + 100, 39: 2 ** 31 - 1, 0: -(2 ** 31)}
    for r, v in bad_rows.items():
        tg[r] = v
    a, b = Scored(x, W, good), Scored(x, W, tg)
    assert a.rc == 0 and b.rc == 0
    rows = torch.tensor(sorted(bad_rows), device=gpu_device)
    keep = torch.ones(T, dtype=torch.bool, device=gpu_device)
    keep[rows] = False
    assert bool(torch.isnan(b.lp[:T][rows]).all())
    assert bool((b.ng[:T][rows] == -1).all()) and bool((b.ne[:T][rows] == -1).all())
    assert torch.equal(a.lp[:T][keep].view(torch.int32), b.lp[:T][keep].view(torch.int32))
    assert torch.equal(a.lse[:T].view(torch.int32), b.lse[:T].view(torch.int32))
    assert torch.equal(a.ng[:T][keep], b.ng[:T][keep]) and torch.equal(a.ne[:T][keep], b.ne[:T][keep])
    assert b.untouched_outside()


# ------------------------------------------------------------------ fixtures, through HipCausalLM.score
_MPATH = f"{GOLDEN}/lm_score_manifest.json"
MANIFEST = json.load(open(_MPATH)) if os.path.exists(_MPATH) else {}
TAGS = sorted(MANIFEST) or ["tiny", "w06", "w17"]


def _fixture(tag):
    from acehip.config import DiTConfig
    from acehip.weights import synth_text_encoder_weights
    from conftest import load_golden
    with safe_open(f"{GOLDEN}/lm_score_{tag}.safetensors", "pt") as f:
        meta = f.metadata()
    cfg = DiTConfig(hidden_size=int(meta["hidden_size"]), intermediate_size=int(meta["intermediate_size"]),
                    num_hidden_layers=int(meta["num_hidden_layers"]),
                    num_attention_heads=int(meta["num_attention_heads"]),
                    num_key_value_heads=int(meta["num_key_value_heads"]), head_dim=int(meta["head_dim"]),
                    rms_norm_eps=float(meta["rms_norm_eps"]), rope_theta=float(meta["rope_theta"]))
    W = synth_text_encoder_weights(cfg, int(meta["vocab_size"]), seed=MANIFEST[tag]["seed"], mode="parity")
    W["embed_tokens.weight"] = W["embed_tokens.weight"] * MANIFEST[tag]["embed_gain"]   # the recorder's gain
    return cfg, W, load_golden(f"lm_score_{tag}")


@pytest.fixture(scope="module", params=TAGS)
def scored(request, gpu_device):
    from acehip.lm import HipCausalLM, HipLMRuntime
    tag = request.param
    cfg, W, g = _fixture(tag)
    S = g["ids"].shape[1]
    rt = HipLMRuntime(cfg, gpu_device.index or 0, max_batch=2, capacity=S + 8, prefill_tokens=2 * (S + 8))
    rt.load({k: v.to(gpu_device) for k, v in W.items()})
    lm = HipCausalLM(rt)
    lp, rank = lm.score(g["ids"].to(gpu_device), int(g["prompt_len"]))
    torch.cuda.synchronize()
    yield tag, lm, g, lp.cpu(), rank.cpu()
    lm.close()


def test_fixture_logprob_rms(scored):
    """Bound: 2 x the manifest's ref_bf16_lp_rms."""
    tag, _, g, lp, _ = scored
    assert lp.dtype == torch.float32 and lp.shape == g["lp_f32"].shape
    rms = float((lp.double() - g["lp_f32"].double()).pow(2).mean().sqrt())
    bound = 2 * MANIFEST[tag]["ref_bf16_lp_rms"]
    print(f"{tag}: log-prob RMS vs fp32 {rms:.5f}, bound {bound:.5f}, "
          f"mean {float(lp.mean()):.5f} vs {float(g['lp_f32'].mean()):.5f}")
    assert rms <= bound, (tag, rms, bound)


def test_fixture_ranks_on_clear_positions(scored):
    tag, _, g, _, rank = scored
    assert rank.dtype == torch.int64
    clear = g["clear"].bool()
    same = rank == g["rank_f32"]
    assert bool(same[clear].all()), (tag, (~same & clear).nonzero().flatten().tolist())


def test_score_leaves_generation_untouched(scored):
    """prefill, two decodes, (score), two decodes: the later logits are bit-identical."""
    tag, lm, g, _, _ = scored
    dev = lm.device
    ids_all = g["ids"].to(dev)
    P = int(g["prompt_len"])
    prompt = torch.cat([ids_all[:, :P], ids_all[:, 5:5 + P]], dim=0)       # two rows
    mask = torch.ones_like(prompt)
    mask[1, :7] = 0
    toks = ids_all[0, P:P + 4]

    def run(with_score):
        out = []
        o = lm(input_ids=prompt, attention_mask=mask, use_cache=True)
        m, past = mask, o.past_key_values
        for i in range(4):
            if with_score and i == 2:
                lm.score(ids_all, P)
            m = torch.cat([m, torch.ones_like(m[:, :1])], dim=1)
            o = lm(input_ids=toks[i].expand(2, 1), past_key_values=past, attention_mask=m, use_cache=True)
            past = o.past_key_values
            out.append(o.logits.clone())
        torch.cuda.synchronize()
        return out, past

    a, _ = run(False)
    gen = lm._generation
    b, past = run(True)
    assert lm._generation == gen + 1 and lm._cache is past and past.length == P + 4
    for i in range(4):
        assert torch.equal(a[i].view(torch.int16), b[i].view(torch.int16)), (tag, i)


# ------------------------------------------------------------------ the seam on the GPU
def test_seam_on_gpu(scored):
    import types
    from acehip.integration import install_lm_score
    from lm_score_ref import StubHandler, StubTokenizer, ids_to_text, recall_from_ranks
    tag, lm, g, lp, rank = scored
    P = int(g["prompt_len"])
    ids = g["ids"][0].tolist()
    calls = []
    mod = types.SimpleNamespace(_calculate_log_prob=lambda *a, **k: calls.append("lp"),
                                _calculate_topk_recall=lambda *a, **k: calls.append("rc"))
    handler = StubHandler(lm, StubTokenizer(), lm.device)
    install_lm_score(handler, mod)
    prompt, target = ids_to_text(ids[:P]), " " + ids_to_text(ids[P:])
    got = mod._calculate_log_prob(handler, prompt, target)
    avg, per_k = mod._calculate_topk_recall(handler, prompt, target, topk=10)
    assert not calls
    assert isinstance(got, float) and got == float(lp.mean())                # the fp32 mean of score()'s rows
    want_avg, want_k = recall_from_ranks(rank.tolist(), 10)
    assert per_k == want_k and abs(avg - want_avg) <= 1e-12
