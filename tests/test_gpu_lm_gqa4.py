"""The 5 Hz LM at heads / kv_heads = 4 on the HIP path (the 4B LM: 32 / 8 heads, hidden 2560,
intermediate 9728), on the fixtures of tools/record_lm_gqa4.py: ``g4tiny`` (4 / 1 heads) and
``w4b`` (the 4B's widths, 2 layers, vocabulary 2048).  The handle sends a ratio-4 stack's prefill
and scoring-forward attention to acehip_attention_extend_bf16 (pos = 0, cap = S) and its decode /
extend steps to the kernels over the cache (csrc/encoder.hip).

Bars, each restated from the test that sets it for the small LMs:
  * logits (tests/test_gpu_lm_decode.py): rel-L2 against the reference's fp32 logits at most twice
    the manifest's ref_bf16_rel_l2, over all calls and over the last quarter; top-1 equal on every
    clear pair; all finite;
  * cache against one use_cache=False call over the final sequence: rel-L2 < 1e-2 (the decode
    attention against the prefill route, both at G = 4);
  * extend in chunks of 1, 5 and the rest against the reference (the same logits rule) and against
    the one-token replay, rel-L2 < 1e-2 (tests/test_gpu_lm_extend.py);
  * score (tests/test_gpu_lm_score.py, tests/test_gpu_lm_extend.py): log-prob RMS against the fp32
    fixture at most twice ref_bf16_lp_rms, ranks equal on every clear position — plain, with
    reuse=False, cold and warm on a runtime with two slots; warm against cold under the same RMS
    bar; a running generation bit-identical with and without scoring calls in between;
  * the handle: a ratio-4 stack with one non-causal layer is refused (ACEHIP_E_ARG), a causal one
    gets a cache, and acehip_enc_forward's last row equals acehip_enc_prefill's output bit for bit.

Measured on an MI355X, rel-L2 over all calls / last quarter / bound, cached vs recomputed and extend
vs one-token steps (bars 1e-2): g4tiny 0.01113 / 0.01137 / 0.02247, 0.00620, 0.00639; w4b 0.01974 /
0.02061 / 0.03948, 0.00927, 0.00993.  w4b scoring: log-prob RMS against the fp32 run 0.16484 (bound
0.32528) plain, cold and warm, mean -7.84214 (fp32 run -7.87160).
"""
import json

import pytest
import torch
from safetensors import safe_open

from conftest import GOLDEN, load_golden, rel_l2

from acehip.config import DiTConfig
from acehip.weights import synth_text_encoder_weights

pytestmark = pytest.mark.gpu

with open(f"{GOLDEN}/lm_gqa4_manifest.json") as _f:
    DEC = json.load(_f)
with open(f"{GOLDEN}/lm_gqa4_score_manifest.json") as _f:
    SCO = json.load(_f)
TAGS = sorted(DEC)
ACEHIP_E_ARG = -1


def _fixture(name, entry):
    with safe_open(f"{GOLDEN}/{name}.safetensors", "pt") as f:
        meta = f.metadata()
    cfg = DiTConfig(hidden_size=int(meta["hidden_size"]), intermediate_size=int(meta["intermediate_size"]),
                    num_hidden_layers=int(meta["num_hidden_layers"]),
                    num_attention_heads=int(meta["num_attention_heads"]),
                    num_key_value_heads=int(meta["num_key_value_heads"]), head_dim=int(meta["head_dim"]),
                    rms_norm_eps=float(meta["rms_norm_eps"]), rope_theta=float(meta["rope_theta"]))
    assert cfg.num_attention_heads == 4 * cfg.num_key_value_heads
    W = synth_text_encoder_weights(cfg, int(meta["vocab_size"]), seed=entry["seed"], mode="parity")
    W["embed_tokens.weight"] = W["embed_tokens.weight"] * entry["embed_gain"]      # the recorder's gain
    return cfg, W, load_golden(name)


def _lm(cfg, W, dev, capacity, max_batch=2, **kw):
    from acehip.lm import HipCausalLM, HipLMRuntime
    rt = HipLMRuntime(cfg, dev.index or 0, max_batch=max_batch, capacity=capacity,
                      prefill_tokens=max_batch * capacity, **kw)
    rt.load({k: v.to(dev) for k, v in W.items()})
    return HipCausalLM(rt)


def _replay(lm, ids, mask, forced):
    """_forward_pass's call sequence; logits[:, -1, :] of every call → [N + 1, B, V] and the final ids / mask."""
    out, past = [], None
    for step in range(forced.shape[1] + 1):
        if past is None:
            o = lm(input_ids=ids, attention_mask=mask, use_cache=True)
        else:
            o = lm(input_ids=ids[:, -1:], past_key_values=past, attention_mask=mask, use_cache=True)
        assert o.logits.shape[:2] == (ids.shape[0], 1) and o.logits.dtype == torch.bfloat16
        out.append(o.logits[:, -1, :])
        past = o.past_key_values
        assert past.get_seq_length() == ids.shape[1]
        if step < forced.shape[1]:
            ids = torch.cat([ids, forced[:, step:step + 1]], dim=1)
            mask = torch.cat([mask, torch.ones_like(mask[:, :1])], dim=1)
    return torch.stack(out), ids, mask


@pytest.fixture(scope="module", params=TAGS)
def replayed(request, gpu_device):
    tag = request.param
    cfg, W, g = _fixture(f"lm_gqa4_{tag}", DEC[tag])
    n = g["ids"].shape[1] + g["forced"].shape[1]
    lm = _lm(cfg, W, gpu_device, capacity=n + 20)
    logits, ids, mask = _replay(lm, g["ids"].to(gpu_device), g["mask"].to(gpu_device), g["forced"].to(gpu_device))
    torch.cuda.synchronize()
    yield tag, lm, g, logits.float().cpu(), ids, mask
    lm.close()


def _check_logits(tag, logits, g):
    ref, bound = g["logits_f32"], 2 * DEC[tag]["ref_bf16_rel_l2"]
    assert logits.shape == ref.shape and torch.isfinite(logits).all()
    err = rel_l2(logits, ref)
    q = logits.shape[0] // 4
    err_q = rel_l2(logits[-q:], ref[-q:])
    print(f"{tag}: rel-L2 {err:.5f} (last quarter {err_q:.5f}), bound {bound:.5f}")
    assert err <= bound, f"{tag}: logits rel-L2 {err:.5f} over all calls, bound {bound:.5f}"
    assert err_q <= bound, f"{tag}: logits rel-L2 {err_q:.5f} over the last quarter, bound {bound:.5f}"
    clear = torch.tensor(DEC[tag]["clear"], dtype=torch.bool)
    assert clear.shape == logits.shape[:2]
    same = logits.argmax(-1) == ref.argmax(-1)
    assert bool(same[clear].all()), f"{tag}: top-1 differs on clear pairs {(~same & clear).nonzero().tolist()}"


def test_logits_vs_reference_fp32(replayed):
    tag, _, g, logits, _, _ = replayed
    _check_logits(tag, logits, g)


def test_cache_vs_recomputation(replayed):
    tag, lm, _, logits, ids, mask = replayed
    o = lm(input_ids=ids, attention_mask=mask, use_cache=False)
    torch.cuda.synchronize()
    assert o.past_key_values is None
    err = rel_l2(o.logits[:, -1, :].float().cpu(), logits[-1])
    print(f"{tag}: cached vs recomputed rel-L2 {err:.5f}")
    assert err < 1e-2, (tag, err)


def test_extend_chunks_vs_single_steps(replayed):
    """After the prompt, the forced tokens in chunks of 1, 5 and the rest with logits="all": row i of
    the chunk at forced offset a is call a + i + 1 of the one-token replay."""
    tag, lm, g, logits, _, _ = replayed
    dev = lm.device
    ids, mask, forced = g["ids"].to(dev), g["mask"].to(dev), g["forced"].to(dev)
    N = forced.shape[1]
    o = lm(input_ids=ids, attention_mask=mask, use_cache=True)
    past, out, a = o.past_key_values, [o.logits[:, -1, :]], 0
    for c in (1, 5, N - 6):
        mask = torch.cat([mask, torch.ones_like(mask[:, :c])], dim=1)
        o = lm.extend(forced[:, a:a + c], past, attention_mask=mask, logits="all")
        assert o.logits.shape[:2] == (2, c) and o.logits.dtype == torch.bfloat16 and o.past_key_values is past
        a += c
        assert past.get_seq_length() == ids.shape[1] + a
        out += [o.logits[:, i, :] for i in range(c)]
    torch.cuda.synchronize()
    assert a == N
    got = torch.stack(out).float().cpu()
    _check_logits(tag, got, g)
    err = rel_l2(got, logits)
    print(f"{tag}: extend vs one-token replay rel-L2 {err:.5f}")
    assert err < 1e-2, (tag, err)
    assert bool((lm._mask[:2, ids.shape[1]:ids.shape[1] + a] == 1).all())


# ------------------------------------------------------------------ scoring, w4b
@pytest.fixture(scope="module")
def scorers(gpu_device):
    cfg, W, g = _fixture("lm_gqa4_score_w4b", SCO["w4b"])
    S = g["ids"].shape[1]
    lms = {slots: _lm(cfg, W, gpu_device, capacity=S + 8, score_slots=slots) for slots in (0, 2)}
    yield lms, g
    for lm in lms.values():
        lm.close()


def _lp_rms(a, b):
    return float((a.double().cpu() - b.double().cpu()).pow(2).mean().sqrt())


def _check_score(g, lp, rank, what):
    lp, rank = lp.cpu(), rank.cpu()
    assert lp.dtype == torch.float32 and lp.shape == g["lp_f32"].shape and rank.dtype == torch.int64
    assert torch.isfinite(lp).all()
    rms, bound = _lp_rms(lp, g["lp_f32"]), 2 * SCO["w4b"]["ref_bf16_lp_rms"]
    print(f"w4b {what}: log-prob RMS vs fp32 {rms:.5f}, bound {bound:.5f}, "
          f"mean {float(lp.mean()):.5f} vs {float(g['lp_f32'].mean()):.5f}")
    assert rms <= bound, (what, rms, bound)
    clear = g["clear"].bool()
    same = rank == g["rank_f32"]
    assert bool(same[clear].all()), (what, (~same & clear).nonzero().flatten().tolist())


def test_score_plain_and_without_reuse(scorers):
    lms, g = scorers
    P = int(g["prompt_len"])
    ids = g["ids"].to(lms[0].device)
    calls = lms[2].score_stats["calls"]
    plain = lms[0].score(ids, P)
    off = lms[2].score(ids, P, reuse=False)
    torch.cuda.synchronize()
    assert lms[2].score_stats["calls"] == calls and lms[0].score_stats["calls"] == 0
    _check_score(g, *plain, "plain")
    assert torch.equal(plain[0].view(torch.int32), off[0].view(torch.int32)) and torch.equal(plain[1], off[1])


def test_score_cold_then_warm_slot(scorers):
    lms, g = scorers
    lm, P = lms[2], int(g["prompt_len"])
    ids = g["ids"].to(lm.device)
    S = ids.shape[1]
    lm.reset_score_cache()
    before = dict(lm.score_stats)
    cold = lm.score(ids, P)
    assert lm.score_stats["last_start"] == 0
    warm = lm.score(ids, P)
    torch.cuda.synchronize()
    st = lm.score_stats
    assert st["last_start"] == P - 1 == 69
    assert st["calls"] == before["calls"] + 2
    assert st["tokens_computed"] == before["tokens_computed"] + S + S - (P - 1)
    assert st["tokens_reused"] == before["tokens_reused"] + P - 1
    _check_score(g, *cold, "cold slot")
    _check_score(g, *warm, "warm slot")
    rms, bound = _lp_rms(warm[0], cold[0]), 2 * SCO["w4b"]["ref_bf16_lp_rms"]
    print(f"w4b warm vs cold: log-prob RMS {rms:.5f}, bound {bound:.5f}")
    assert rms <= bound, (rms, bound)


def test_score_leaves_generation_untouched(scorers):
    """prefill, two decodes, (a plain, a cold and a warm reusing score), two decodes: the later
    logits are bit-identical to the run without scoring."""
    lms, g = scorers
    lm = lms[2]
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
                lm.reset_score_cache()
                lm.score(ids_all, P, reuse=False)
                lm.score(ids_all[:, :100], P)
                assert lm.score_stats["last_start"] == 0
                lm.score(ids_all, P)
                assert lm.score_stats["last_start"] == P - 1
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
        assert torch.equal(a[i].view(torch.int16), b[i].view(torch.int16)), i


# ------------------------------------------------------------------ the handle
def _enc_create(ff, cfg, kinds, out_dim=0, max_tokens=256, max_S=128):
    sl = (ff.c_uint8 * len(kinds))(*kinds)
    c = ff.EncCfg(hidden=cfg.hidden_size, intermediate=cfg.intermediate_size, heads=cfg.num_attention_heads,
                  kv_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, layers=len(kinds), window=8, in_dim=0,
                  embed_bias=0, out_dim=out_dim, eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta,
                  max_tokens=max_tokens, max_S=max_S, sliding=ff.ctypes.cast(sl, ff.POINTER(ff.c_uint8)))
    h = ff.c_void_p()
    rc = ff.lib().acehip_enc_create(0, ff.ctypes.byref(c), ff.ctypes.byref(h))
    return rc, h


def test_handle_refuses_non_causal_ratio_4_stacks(gpu_device):
    from acehip import _ffi as ff
    cfg, _, _ = _fixture("lm_gqa4_g4tiny", DEC["g4tiny"])
    for kinds, out_dim in (([2, 1, 2], 0), ([2, 2, 0], 0), ([2, 2, 2], 64)):
        rc, h = _enc_create(ff, cfg, kinds, out_dim)
        assert rc == ACEHIP_E_ARG and not h.value, (kinds, out_dim, rc)
        assert b"unsupported dims" in ff.lib().acehip_last_error()
    rc, h = _enc_create(ff, cfg, [2, 2, 2])
    assert rc == 0 and h.value
    assert ff.lib().acehip_enc_kv_create(h, 2, 128) == 0           # a causal ratio-4 stack gets a cache
    assert ff.lib().acehip_enc_destroy(h) == 0


def test_forward_last_row_equals_prefill(replayed):
    """acehip_enc_forward (every row, no cache) and acehip_enc_prefill (the last row, K / V to the
    cache) run the same launches: bit-equal on the fixture's prompt, left-padding mask included,
    and without a mask."""
    tag, lm, g, _, _, _ = replayed
    rt = lm.rt
    ids = g["ids"].to(lm.device)
    x = rt.embed(ids)
    km = (g["mask"] != 0).to(device=lm.device, dtype=torch.uint8).contiguous()
    for mask in (km, None):
        full = rt.stack.forward(x, mask)
        last = rt.prefill(x, mask)
        torch.cuda.synchronize()
        assert full.shape == x.shape and torch.isfinite(last.float()).all()
        assert torch.equal(full[:, -1].contiguous().view(torch.int16), last.view(torch.int16)), (tag, mask is None)
