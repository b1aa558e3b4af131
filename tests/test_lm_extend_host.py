"""HipCausalLM.extend and the slot logic of HipCausalLM.score on the host (no GPU), with the runtime
replaced by a torch fp32 stand-in that keeps, per cache row, the embeddings it was given and
recomputes the wrapped transformers model over them.  The stand-in proves the wrapper — mask and
id columns, the ticket, the contract errors, the fallback, which slot a scoring call takes and
from which position it continues — not the kernels (tests/test_gpu_lm_extend.py does that)."""
import json

import pytest
import torch
from safetensors import safe_open

from conftest import GOLDEN, load_golden

from acehip.config import DiTConfig
from acehip.lm import HipCausalLM, HipKVCache
from acehip.weights import synth_text_encoder_weights
from lm_score_ref import build_model

CFG = dict(vocab_size=97, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
           num_key_value_heads=1, head_dim=32, rms_norm_eps=1e-6, rope_theta=10000.0, max_position_embeddings=256,
           attention_bias=False, use_sliding_window=False, tie_word_embeddings=True)


def _model():
    import transformers
    torch.manual_seed(0)
    return transformers.Qwen3ForCausalLM(transformers.Qwen3Config(**CFG)).eval()


class RowRuntime:
    """Stand-in for acehip.lm.HipLMRuntime: cache row r is the list of embeddings fed at positions
    0, 1, ... of that row; every call recomputes the model over a row's whole history.
    ``fail_extend``: raise the RuntimeError an acehip call would, on the extend calls so numbered."""

    def __init__(self, model, max_batch=2, capacity=64, score_slots=0, prefill_tokens=None, fail_extend=()):
        self.model, self.device = model, torch.device("cpu")
        self.max_batch, self.capacity, self.score_slots = max_batch, capacity, score_slots
        self.prefill_tokens = prefill_tokens
        self.rows = [None] * (max_batch + score_slots)
        self.fail_extend, self.n_extend = set(fail_extend), 0
        self.calls = []

    def embed(self, ids):
        return self.model.model.embed_tokens(ids)

    def _run(self, row0, B, kmask, n):
        x = torch.stack([self.rows[row0 + b] for b in range(B)])
        L = x.shape[1]
        m = None if kmask is None else kmask[:B, :L].long()
        with torch.no_grad():
            return self.model.model(inputs_embeds=x, attention_mask=m).last_hidden_state[:, L - n:]

    def extend(self, x, kmask, row0, pos):
        self.n_extend += 1
        self.calls.append(("extend", tuple(x.shape[:2]), row0, pos))
        if self.n_extend in self.fail_extend:
            raise RuntimeError("acehip enc_extend failed (-3): injected")
        B, n = x.shape[:2]
        assert row0 >= 0 and row0 + B <= len(self.rows) and pos + n <= self.capacity
        for b in range(B):
            old = self.rows[row0 + b]
            assert pos == 0 or (old is not None and old.shape[0] >= pos), "continues past what the row holds"
            self.rows[row0 + b] = x[b].detach().clone() if pos == 0 else torch.cat([old[:pos], x[b].detach()])
        return self._run(row0, B, kmask, n)

    def prefill(self, x, kmask):
        self.calls.append(("prefill", tuple(x.shape[:2])))
        for b in range(x.shape[0]):
            self.rows[b] = x[b].detach().clone()
        return self._run(0, x.shape[0], kmask, 1)[:, 0]

    def decode(self, x, kmask, pos):
        self.calls.append(("decode", pos))
        for b in range(x.shape[0]):
            self.rows[b] = torch.cat([self.rows[b][:pos], x[b:b + 1].detach()])
        return self._run(0, x.shape[0], kmask, 1)[:, 0]

    def lm_head(self, h):
        assert h.shape[0] <= 16
        with torch.no_grad():
            return self.model.lm_head(h)

    def forward_all(self, x):
        self.calls.append(("forward_all", tuple(x.shape[:2])))
        with torch.no_grad():
            return self.model.model(inputs_embeds=x).last_hidden_state

    def score_rows(self, h, targets):
        with torch.no_grad():
            logits = self.model.lm_head(h).float()
        tl = logits.gather(1, targets[:, None])
        lse = torch.logsumexp(logits, dim=1)
        col = torch.arange(logits.shape[1])[None, :]
        ng = (logits > tl).sum(1).to(torch.int32)
        ne = ((logits == tl) & (col < targets[:, None])).sum(1).to(torch.int32)
        return tl[:, 0] - lse, lse, ng, ne


def _prompt():
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, CFG["vocab_size"], (2, 11), generator=g)
    mask = torch.ones(2, 11, dtype=torch.long)
    mask[1, :4] = 0                                   # left-padded row
    more = torch.randint(1, CFG["vocab_size"], (2, 26), generator=g)
    return ids, mask, more


# ------------------------------------------------------------------ extend
def test_extend_in_chunks_equals_the_model():
    model = _model()
    ids, mask, more = _prompt()
    full_ids = torch.cat([ids, more], 1)
    full_mask = torch.cat([mask, torch.ones_like(more)], 1)
    with torch.no_grad():
        want = model(input_ids=full_ids, attention_mask=full_mask).logits
    rt = RowRuntime(model)
    lm = HipCausalLM(rt, wrapped=model, fallback=True)        # fallback: the id columns are kept
    o = lm(input_ids=ids, attention_mask=mask, use_cache=True)
    past = o.past_key_values
    assert torch.allclose(o.logits[:, 0], want[:, 10], atol=1e-5)
    a = 0
    for c, how in ((1, "all"), (3, "last"), (17, "all"), (4, "all")):       # 17 x 2 rows: lm_head in slices
        L = 11 + a + c
        o = lm.extend(more[:, a:a + c], past, attention_mask=full_mask[:, :L], logits=how)
        assert o.past_key_values is past and past.get_seq_length() == L and lm._cache is past
        keep = c if how == "all" else 1
        assert o.logits.shape == (2, keep, CFG["vocab_size"])
        assert torch.allclose(o.logits, want[:, L - keep:L], atol=1e-5), (c, how)
        a += c
        assert torch.equal(lm._mask[:2, :L].long(), full_mask[:, :L]) and torch.equal(lm._ids[:2, :L], full_ids[:, :L])
    assert bool((lm._mask[:2, 11 + a:] == 0).all())
    assert [c[0] for c in rt.calls] == ["prefill"] + ["extend"] * 4
    assert rt.calls[3] == ("extend", (2, 17), 0, 15)
    # a one-token __call__ continues the same ticket
    o = lm(input_ids=more[:, a:a + 1], past_key_values=past, attention_mask=full_mask[:, :12 + a])
    assert past.get_seq_length() == 12 + a
    with torch.no_grad():
        w2 = model(input_ids=full_ids[:, :12 + a], attention_mask=full_mask[:, :12 + a]).logits[:, -1]
    assert torch.allclose(o.logits[:, 0], w2, atol=1e-5)
    # without a mask every new column is admitted
    lm2 = HipCausalLM(RowRuntime(model))
    p2 = lm2(input_ids=ids[:1]).past_key_values
    o = lm2.extend(more[:1, :5], p2, logits="all")
    with torch.no_grad():
        w3 = model(input_ids=torch.cat([ids[:1], more[:1, :5]], 1)).logits[:, -5:]
    assert torch.allclose(o.logits, w3, atol=1e-5) and bool((lm2._mask[0, :16] == 1).all())


def test_extend_contract_errors():
    model = _model()
    ids, mask, more = _prompt()
    lm = HipCausalLM(RowRuntime(model, capacity=16))
    other = HipCausalLM(RowRuntime(model, capacity=16))
    old = lm(input_ids=ids, attention_mask=mask).past_key_values
    past = lm(input_ids=ids, attention_mask=mask).past_key_values
    tok = more[:, :3]
    with pytest.raises(ValueError, match="foreign"):
        lm.extend(tok, HipKVCache(other, 1, 2, 11))
    with pytest.raises(ValueError, match="foreign"):
        lm.extend(tok, None)
    with pytest.raises(ValueError, match="stale"):
        lm.extend(tok, old)
    with pytest.raises(ValueError, match="batch"):
        lm.extend(tok[:1], past)
    with pytest.raises(ValueError, match="exceed"):
        lm.extend(more[:, :6], past)                      # 11 + 6 > 16
    with pytest.raises(ValueError, match="attention_mask"):
        lm.extend(tok, past, attention_mask=torch.ones(2, 13, dtype=torch.long))
    with pytest.raises(ValueError, match="logits"):
        lm.extend(tok, past, logits="first")
    with pytest.raises(ValueError, match="input_ids"):
        lm.extend(tok[:, :0], past)
    with pytest.raises(ValueError, match="new tokens"):
        lm(input_ids=tok, past_key_values=past)           # __call__ is unchanged
    assert past.length == 11 and lm._cache is past
    m = torch.cat([mask, torch.ones(2, 5, dtype=torch.long)], 1)
    o = lm.extend(more[:, :5], past, attention_mask=m)    # fills the cache exactly
    with torch.no_grad():
        want = model(input_ids=torch.cat([ids, more[:, :5]], 1), attention_mask=m).logits[:, -1:]
    assert past.length == 16 and torch.allclose(o.logits, want, atol=1e-5)
    with pytest.raises(ValueError, match="exceed"):
        lm.extend(tok[:, :1], past)


def test_extend_fallback_hands_over_the_whole_sequence():
    model = _model()
    ids, mask, more = _prompt()
    seen = []

    class Spy(torch.nn.Module):
        config = model.config

        def forward(self, **kw):
            seen.append(kw["input_ids"].clone())
            return model(**kw)

    rt = RowRuntime(model, fail_extend={2})
    lm = HipCausalLM(rt, wrapped=Spy(), fallback=True)
    past = lm(input_ids=ids, attention_mask=mask).past_key_values
    m = torch.cat([mask, torch.ones(2, 3, dtype=torch.long)], 1)
    lm.extend(more[:, :3], past, attention_mask=m)
    m = torch.cat([m, torch.ones(2, 4, dtype=torch.long)], 1)
    o = lm.extend(more[:, 3:7], past, attention_mask=m, logits="all")         # the failing call
    assert len(seen) == 1 and torch.equal(seen[0], torch.cat([ids, more[:, :7]], 1))
    with torch.no_grad():
        want = model(input_ids=seen[0], attention_mask=m).logits
    assert torch.allclose(o.logits, want[:, -4:], atol=1e-5)
    assert lm._delegating and not isinstance(o.past_key_values, HipKVCache)
    # the rest of the generation runs on the wrapped module, with its own cache
    m = torch.cat([m, torch.ones(2, 2, dtype=torch.long)], 1)
    o2 = lm.extend(more[:, 7:9], o.past_key_values, attention_mask=m, logits="all")
    with torch.no_grad():
        want2 = model(input_ids=torch.cat([ids, more[:, :9]], 1), attention_mask=m).logits[:, -2:]
    assert torch.allclose(o2.logits, want2, atol=1e-5) and rt.n_extend == 2
    # without fallback the error surfaces
    lm3 = HipCausalLM(RowRuntime(model, fail_extend={1}), wrapped=model)
    p3 = lm3(input_ids=ids, attention_mask=mask).past_key_values
    with pytest.raises(RuntimeError, match="injected"):
        lm3.extend(more[:, :3], p3)


# ------------------------------------------------------------------ the slot logic of score
with open(f"{GOLDEN}/lm_score_manifest.json") as _f:
    MANIFEST = json.load(_f)


@pytest.fixture(scope="module")
def tiny():
    with safe_open(f"{GOLDEN}/lm_score_tiny.safetensors", "pt") as f:
        meta = f.metadata()
    cfg = DiTConfig(hidden_size=int(meta["hidden_size"]), intermediate_size=int(meta["intermediate_size"]),
                    num_hidden_layers=int(meta["num_hidden_layers"]),
                    num_attention_heads=int(meta["num_attention_heads"]),
                    num_key_value_heads=int(meta["num_key_value_heads"]), head_dim=int(meta["head_dim"]),
                    rms_norm_eps=float(meta["rms_norm_eps"]), rope_theta=float(meta["rope_theta"]))
    W = synth_text_encoder_weights(cfg, int(meta["vocab_size"]), seed=MANIFEST["tiny"]["seed"], mode="parity")
    g = load_golden("lm_score_tiny")
    return build_model(meta, W), g["ids"], int(g["prompt_len"])


def _other(ids, lo, hi, vocab, seed):
    """A copy of ids [1, S] whose tokens [lo, hi) are replaced, every one by a different token."""
    g = torch.Generator().manual_seed(seed)
    out = ids.clone()
    out[0, lo:hi] = (ids[0, lo:hi] + torch.randint(1, vocab, (hi - lo,), generator=g)) % vocab
    return out


def _scorer(model, slots, **kw):
    rt = RowRuntime(model, capacity=128, score_slots=slots, **kw)
    return HipCausalLM(rt), rt


def _same(a, b):
    return torch.allclose(a[0], b[0], atol=1e-5) and torch.equal(a[1], b[1])


def test_score_slots_starts_and_results(tiny):
    model, ids, P = tiny
    S, V = ids.shape[1], model.config.vocab_size
    plain, prt = _scorer(model, 0)
    want = plain.score(ids, P)
    want30 = plain.score(ids[:, :100], P)
    assert [c[0] for c in prt.calls] == ["forward_all"] * 2 and plain.score_stats["calls"] == 0

    # (a), (b): cold on the truncated sequence, then the whole one from the prompt's last position
    lm, rt = _scorer(model, 2)
    state = (lm._generation, lm._cache, lm._masked, lm._mask.clone())
    assert _same(lm.score(ids[:, :100], P), want30) and lm.score_stats["last_start"] == 0
    assert _same(lm.score(ids, P), want) and lm.score_stats["last_start"] == P - 1 == 69
    assert rt.calls == [("extend", (1, 100), 2, 0), ("extend", (1, S - 69), 2, 69)]
    assert lm.score_stats == {"calls": 2, "tokens_computed": 100 + S - 69, "tokens_reused": 69, "last_start": 69}
    # the same sequence again: everything before the prompt's last position is reused
    assert _same(lm.score(ids, P), want) and lm.score_stats["last_start"] == 69 and rt.calls[-1][2] == 2
    # reuse=False takes forward_all and counts nothing
    assert _same(lm.score(ids, P, reuse=False), want)
    assert rt.calls[-1][0] == "forward_all" and lm.score_stats["calls"] == 3
    assert (lm._generation, lm._cache, lm._masked) == state[:3] and torch.equal(lm._mask, state[3])
    assert rt.rows[0] is None and rt.rows[1] is None          # the generation's rows were never written

    # (c): one slot holds a sequence that differs from token 40 on
    lm, rt = _scorer(model, 1)
    lm.score(_other(ids, 40, S, V, 5), P)
    assert _same(lm.score(ids, P), want) and lm.score_stats["last_start"] == 40
    assert rt.calls[-1] == ("extend", (1, S - 40), 2, 40)

    # (d): X with another target, an unrelated Y, then X
    for slots, start, row in ((2, 69, 2), (1, 0, 2)):
        lm, rt = _scorer(model, slots)
        lm.score(_other(ids, P, S, V, 6), P)
        lm.score(_other(ids, 0, S, V, 7), P)
        assert lm.score_stats["last_start"] == 0 and rt.calls[-1][2] == 2 + (slots - 1)
        assert _same(lm.score(ids, P), want)
        assert lm.score_stats["last_start"] == start and rt.calls[-1] == ("extend", (1, S - start), row, start)


def test_score_slots_lru_failure_and_reset(tiny):
    model, ids, P = tiny
    S, V = ids.shape[1], model.config.vocab_size
    plain, _ = _scorer(model, 0)
    want = plain.score(ids, P)
    A, B, C = _other(ids, 0, S, V, 1), _other(ids, 0, S, V, 2), _other(ids, 0, S, V, 3)
    assert len({int(t[0, 0]) for t in (ids, A, B, C)}) == 4  # no two share a first token

    lm, rt = _scorer(model, 2)
    for seq, row in ((A, 2), (B, 3), (A, 2), (C, 3), (B, 2)):    # the least recently used slot goes
        lm.score(seq, P)
        assert rt.calls[-1][2] == row, (rt.calls, row)
    assert [c[3] for c in rt.calls] == [0, 0, 69, 0, 0]
    # a partial match yields to an empty slot, so two prompts with a common prefix keep a slot each
    lm, rt = _scorer(model, 2)
    X, Y = ids, _other(ids, 20, S, V, 4)
    for seq, row, start in ((X, 2, 0), (Y, 3, 0), (X, 2, 69), (Y, 3, 69)):
        lm.score(seq, P)
        assert rt.calls[-1][2:] == (row, start)
    lm.score(_other(ids, 30, S, V, 8), P)                     # no empty slot left: the longer prefix wins
    assert rt.calls[-1][2:] == (2, 30)

    # a failing extend leaves its slot empty: the next call is cold, and right
    lm, rt = _scorer(model, 1, fail_extend={2})
    lm.score(ids[:, :100], P)
    with pytest.raises(RuntimeError, match="injected"):
        lm.score(ids, P)
    assert lm._slot_ids == [None] and lm.score_stats["calls"] == 1     # the stats count what succeeded
    assert _same(lm.score(ids, P), want) and lm.score_stats["last_start"] == 0
    assert _same(lm.score(ids, P), want) and lm.score_stats["last_start"] == 69
    lm.reset_score_cache()
    assert lm._slot_ids == [None]
    assert _same(lm.score(ids, P), want) and lm.score_stats["last_start"] == 0
    # a runtime that reloads its cache (cache_epoch) empties the slots too
    rt.cache_epoch = 1
    assert _same(lm.score(ids, P), want) and lm.score_stats["last_start"] == 0
    assert _same(lm.score(ids, P), want) and lm.score_stats["last_start"] == 69
    # the argument checks come first
    with pytest.raises(ValueError, match="prompt_len"):
        lm.score(ids, 0)
    with pytest.raises(ValueError, match="capacity"):
        _scorer(model, 1)[0].score(torch.cat([ids, ids], 1), P)
