"""What the LM's top-k / top-p logit filters compute (helper module, not a test).

Two statements of the same semantics, used by tests/test_lm_filter_host.py,
tests/test_gpu_lm_filter.py, tools/record_lm_filter.py and tools/bench_lm_filter.py:

  * the fp32 torch chain of ``LLMHandler._apply_top_k_filter`` / ``_apply_top_p_filter``
    (acestep/llm_inference.py:367-372, :374-385), restated: top-k compares against the k-th value
    of ``topk``; top-p sorts descending, takes the softmax of the sorted values in fp32, an
    inclusive scan, ``> top_p``, shifts the flags one rank down (rank 0 always kept) and scatters
    them back.  This is what the token loop runs without acehip.
  * the contract in fp64: with p = softmax(row) and the entries ranked by value, descending, equal
    values in index order, rank 0 is kept and rank i >= 1 is kept iff the p of ranks < i sums to
    <= q.  ``n64(row, q)`` is the number kept, ``mask64`` the kept set.

DELTA bounds what fp32 rounding may move: a summation whose longest dependent chain has 1024
terms has relative error <= 1024 * 2^-24 = 6.1e-5 on a mass <= 1; the few ulps of exp and of the
division fit in the rest of 1e-4.  A row is *gapped* at top_p when n64(row, top_p - DELTA) ==
n64(row, top_p + DELTA) and the last kept value differs from the first removed one: then every
implementation inside the bound keeps the same set, whatever its order among equal values.
"""
import torch

DELTA = 1e-4
NEG_INF = float("-inf")


# ------------------------------------------------------------------ the fp32 torch chain
def torch_top_k(logits: torch.Tensor, top_k) -> torch.Tensor:
    """llm_inference.py:367-372, in place."""
    if top_k is not None and top_k > 0:
        kth = torch.topk(logits, top_k)[0][..., -1, None]
        logits[logits < kth] = NEG_INF
    return logits


def torch_top_p(logits: torch.Tensor, top_p) -> torch.Tensor:
    """llm_inference.py:374-385, in place."""
    if top_p is not None and 0.0 < top_p < 1.0:
        sorted_logits, sorted_idx = torch.sort(logits, descending=True)
        cum = torch.cumsum(torch.softmax(sorted_logits.float(), dim=-1), dim=-1)
        remove = cum > top_p
        remove[..., 1:] = remove[..., :-1].clone()
        remove[..., 0] = 0
        logits[remove.scatter(1, sorted_idx, remove)] = NEG_INF
    return logits


# ------------------------------------------------------------------ the contract in fp64
def ranked64(row: torch.Tensor):
    """One row → (order, exclusive prefix mass in fp64): ``order[i]`` is the index of rank i
    (value descending, equal values by index), ``mass[i]`` the softmax mass of ranks < i."""
    assert row.dim() == 1
    x = row.detach().double().cpu()
    order = torch.sort(x, descending=True, stable=True)[1]
    v = x[order]
    live = torch.isfinite(v)
    if not bool(live.any()):
        return order, None
    e = torch.where(live, torch.exp(v - v[0]), torch.zeros_like(v))
    p = e / e.sum()
    return order, torch.cumsum(p, 0) - p


def n64(row: torch.Tensor, q: float) -> int:
    """Entries the contract keeps at threshold q (0 for a row with no finite entry: nothing is
    ranked, the row is left alone)."""
    order, mass = ranked64(row)
    if mass is None:
        return 0
    live = torch.isfinite(row.detach().double().cpu()[order])
    return max(1, int(((mass <= q) & live).sum()))


def band64(row: torch.Tensor, top_p: float, delta: float = DELTA):
    """(n64(row, top_p − delta), n64(row, top_p + delta)) from one ranking."""
    order, mass = ranked64(row)
    if mass is None:
        return 0, 0
    live = torch.isfinite(row.detach().double().cpu()[order])
    return tuple(max(1, int(((mass <= q) & live).sum())) for q in (top_p - delta, top_p + delta))


def mask64(row: torch.Tensor, q: float) -> torch.Tensor:
    """The kept set at threshold q as a bool mask over the row (−inf entries are not 'kept':
    they stay −inf either way); None for a row with no finite entry."""
    order, mass = ranked64(row)
    if mass is None:
        return None
    keep = torch.zeros(row.numel(), dtype=torch.bool)
    keep[order[:n64(row, q)]] = True
    return keep


def gapped(row: torch.Tensor, top_p: float, delta: float = DELTA) -> bool:
    order, mass = ranked64(row)
    if mass is None:
        return True
    v = row.detach().double().cpu()[order]
    lo, hi = (max(1, int(((mass <= q) & torch.isfinite(v)).sum())) for q in (top_p - delta, top_p + delta))
    if lo != hi:
        return False
    return lo >= v.numel() or bool(v[lo - 1] > v[lo])


def kept_count(out_row: torch.Tensor) -> int:
    return int(torch.isfinite(out_row.detach().float().cpu()).sum())


# ------------------------------------------------------------------ rows
def codes_phase_row(V: int, sigma: float, seed: int, finite: int = 65268, dtype=torch.float32) -> torch.Tensor:
    """The codes-phase pattern: only the last ``finite`` ids are finite (the FSM has masked the rest)."""
    g = torch.Generator().manual_seed(seed)
    row = torch.randn(V, generator=g) * sigma
    row[:max(V - finite, 0)] = NEG_INF
    return row.to(dtype)


def scattered_row(V: int, sigma: float, seed: int, masked: int, dtype=torch.float32) -> torch.Tensor:
    """randn·σ with ``masked`` entries at random positions set to −inf."""
    g = torch.Generator().manual_seed(seed)
    row = torch.randn(V, generator=g) * sigma
    row[torch.randperm(V, generator=g)[:masked]] = NEG_INF
    return row.to(dtype)
