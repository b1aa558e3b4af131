"""What the score-range tests of the attention kernels share (tests/test_attn_ranges_host.py on the
CPU, tests/test_gpu_attn_ranges.py on the GPU): "hard" inputs whose scores span tens of nats along
the key axis, an fp64 reference, a tile-by-tile model of the flash kernels' arithmetic, two mutants
of that model, and the per-row criterion.

Inputs.  q, k and v start as randn (fixed seed, CPU generator).  The random parts of q and k are
made orthogonal to a unit vector u; key j then gets c(j)·u and query row i gets a_i·u with a_i
cycling over {+a, −a, 0, a/2} by i mod 4, so the score of (i, j) is the randn score plus
scale·a_i·c(j): rows that rise, fall, stay flat and half-rise sit side by side inside one 32-row
wave.  c is a ramp over the keys, a sawtooth whose period (37, 45, 150, 333: chosen per case) is no
multiple of the 64-key tile, so that band windows and causal prefixes meet rises and drops at every
offset within a tile, or half of each; `height` is the rise in nats that a +a row sees over the
profile's full swing, tuned per case until tests/test_attn_ranges_host.py's input conditions hold.  In the cross-fused
entry q is the output of a projection and a q-norm and is left alone: only the cached k gets c(j)·u
(with a = 1), and q·u varies by row on its own.

Model.  `tile_walk` does in fp32 what attn_wave_tile (csrc/attn_tile.h), attn_pw_kernel and
attn_small_kernel do per query row: 64-key tiles from key 0, masked keys at the sentinel NEG (keys
past Sk at PAST), the reference max moved only when a tile's max exceeds it by more than TAU = 8
log2 units, l summed from the fp32 P, O += bf16(P)·V, O·alpha and l·alpha on a move, O / l rounded
to bf16 at the end.  It differs from a kernel in the fp32 summation order, a 1-ulp exp2, and where a
split route cuts the key range; none of these changes the size of the bf16 roundings of P and O.

Criterion.  Per (batch, head, query row): ‖got − ref‖₂ / ‖ref‖₂ over the row's 128 outputs against
the fp64 reference.  A case passes when every row is within MARGIN = 2 times the model's worst row
on the same inputs: a row's error is the RMS of about 128 independent roundings, and the model's own
rows spread about a factor 1.8 around their mean, so another summation order stays inside 2."""
import functools
from dataclasses import dataclass

import torch

SCALE = 128 ** -0.5
TILE, TAU = 64, 8.0
NEG, PAST = -2.0 ** 100, -2.0 ** 126        # csrc/attn_tile.h
LOG2E = 1.4426950408889634
MARGIN = 2.0
CROSS_D, CROSS_EPS = 256, 1e-6


@dataclass(frozen=True)
class Case:
    """One input set.  entry: attn | masked | decode | extend | cross | probs.  window: −1 full,
    ≥ 0 band |i − j| ≤ window, −2 causal.  valid: per batch row, the number of unpadded keys
    (masked).  pos: extend's first new cache position (Sq new queries, Sk = pos + Sq keys)."""
    name: str
    entry: str
    B: int
    H: int
    KV: int
    Sq: int
    Sk: int
    window: int = -1
    valid: tuple = ()
    pos: int = 0
    height: float = 20.0
    profile: str = "ramp"
    a: float = 8.0
    seed: int = 0
    period: int = 37


def key_profile(profile, n, period=37):
    """c(j) / max c over the n keys, in [0, 1]."""
    j = torch.arange(n, dtype=torch.float32)
    ramp = j / max(n - 1, 1)
    saw = (j % period) / (period - 1)
    return {"ramp": ramp, "saw": saw, "mix": 0.5 * (ramp + saw)}[profile]


def _orth(x, u):
    return x - (x @ u)[..., None] * u


def cross_q(xn, wq, qnw, B, S, H):
    """The q the cross-Q projection's head-post epilogue writes (csrc/headpost.h): the projection,
    the normalised value and the weighted value are each rounded to bf16.  → [B, H, S, 128]."""
    q = (xn.float() @ wq.float().T).bfloat16().float().view(B, S, H, 128)
    q = (q * torch.rsqrt(q.pow(2).mean(-1, keepdim=True) + CROSS_EPS)).bfloat16().float() * qnw.float()
    return q.bfloat16().permute(0, 2, 1, 3).contiguous()


def make_inputs(case, hard=True):
    """bf16 (q, k, v) of a case on the CPU, q [B, H, Sq, 128], k / v [B, KV, Sk, 128]; hard = False
    leaves out the u components (the suite's usual randn inputs, same seed).  The cross entry also
    returns the projection's operands under "xn", "wq", "qnw"."""
    c = case
    g = torch.Generator().manual_seed(7919 * c.seed + 131 * c.Sq + c.Sk + c.H)
    u = torch.randn(128, generator=g)
    u = u / u.norm()
    extra = {}
    if c.entry == "cross":
        xn = torch.randn(c.B * c.Sq, CROSS_D, generator=g).bfloat16()
        wq = (torch.randn(c.H * 128, CROSS_D, generator=g) * 0.05).bfloat16()
        qnw = (1.0 + 0.1 * torch.randn(128, generator=g)).bfloat16()
        q = cross_q(xn, wq, qnw, c.B, c.Sq, c.H)
        extra = dict(xn=xn, wq=wq, qnw=qnw)
    else:
        q = _orth(torch.randn(c.B, c.H, c.Sq, 128, generator=g), u)
    k = _orth(torch.randn(c.B, c.KV, c.Sk, 128, generator=g), u)
    v = torch.randn(c.B, c.KV, c.Sk, 128, generator=g)
    if hard:
        a = 1.0 if c.entry == "cross" else c.a
        k = k + (c.height / (SCALE * a)) * key_profile(c.profile, c.Sk, c.period)[:, None] * u
        if c.entry != "cross":
            cyc = torch.tensor([a, -a, 0.0, 0.5 * a])
            rows = torch.arange(c.Sq) if c.Sq > 1 else torch.arange(c.H)[:, None]     # decode: by head
            q = q + cyc[rows % 4][..., None] * u
    if c.entry != "cross":
        q = q.bfloat16()
    return dict(q=q, k=k.bfloat16(), v=v.bfloat16(), **extra)


def admit(case):
    """ok[b, 0, i, j]: query i admits key j (bool [B, 1, Sq, Sk]), by the entry's documented mask."""
    c = case
    i = torch.arange(c.Sq)[:, None]
    j = torch.arange(c.Sk)[None, :]
    ok = torch.ones(c.Sq, c.Sk, dtype=torch.bool)
    if c.entry == "extend":
        ok = j <= c.pos + i
    elif c.window >= 0:
        ok = (i - j).abs() <= c.window
    elif c.window == -2:
        ok = j <= i
    ok = ok[None, None].expand(c.B, 1, c.Sq, c.Sk).clone()
    if c.valid:
        for b, n in enumerate(c.valid):
            ok[b, :, :, n:] = False
    return ok


def reference(q, k, v, ok, scale=SCALE):
    """fp64 softmax(scale·q·kᵀ + mask)·v → [B, H, Sq, 128].  A masked key weighs nothing; a row
    without an admissible key (the key-padding entry's finite additive mask) is uniform over Sk."""
    G = q.shape[1] // k.shape[1]
    s = (q.double() @ k.double().repeat_interleave(G, 1).transpose(2, 3)) * scale
    s = s.masked_fill(~ok, -1e30)
    return torch.softmax(s, -1) @ v.double().repeat_interleave(G, 1)


def reference_probs(q, k, scale=SCALE):
    """fp64 softmax rows [B, H, Sq, Sk] (acehip_attention_probs_bf16 never masks)."""
    G = q.shape[1] // k.shape[1]
    return torch.softmax((q.double() @ k.double().repeat_interleave(G, 1).transpose(2, 3)) * scale, -1)


def model_probs(q, k, scale=SCALE):
    """attn_probs_kernel's arithmetic: fp32 scores, exact row max, exp2, one division, one bf16
    rounding of each stored value."""
    G = q.shape[1] // k.shape[1]
    s = (q.float() @ k.float().repeat_interleave(G, 1).transpose(2, 3)) * (scale * LOG2E)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return (p / p.sum(-1, keepdim=True)).bfloat16().float()


def tile_walk(q, k, v, ok, scale=SCALE, mutant=0):
    """The flash kernels' per-row arithmetic (module docstring).  mutant 1: alpha is not applied to
    O columns 96..127 once the row's accumulator is non-empty; mutant 2: there, O takes the alpha
    of the neighbouring row (i ^ 1).  → dict: out [B, H, Sq, 128] (bf16 values as fp32) and, per
    row and tile [B, H, Sq, tiles], rescale (the max moved with a non-empty accumulator), lazy (the
    tile max was more than 1 log2 unit above the reference max and it did not move), relevant
    (rescale whose mass before it was 10 % .. 90 % of the row's final l); tiles_seen [B, H, Sq]."""
    B, H, Sq, _ = q.shape
    Sk = k.shape[2]
    G = H // k.shape[1]
    nt = -(-Sk // TILE)
    pad = nt * TILE - Sk
    s = q.float() @ k.float().repeat_interleave(G, 1).transpose(2, 3)
    s = torch.where(ok.expand(B, H, Sq, Sk), s, torch.tensor(NEG))
    s = torch.nn.functional.pad(s, (0, pad), value=PAST)
    okp = torch.nn.functional.pad(ok.expand(B, H, Sq, Sk), (0, pad), value=False)
    vv = torch.nn.functional.pad(v.float().repeat_interleave(G, 1), (0, 0, 0, pad))
    sl2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    m = torch.full((B, H, Sq), NEG)
    l = torch.zeros(B, H, Sq)
    O = torch.zeros(B, H, Sq, 128)
    seen = torch.zeros(B, H, Sq, dtype=torch.bool)
    axis = 2 if Sq > 1 else 1
    n_ax = q.shape[axis]
    nb = torch.arange(n_ax) ^ 1
    nb = torch.where(nb < n_ax, nb, torch.arange(n_ax))
    ev = {n_: torch.zeros(B, H, Sq, nt, dtype=torch.bool) for n_ in ("rescale", "lazy")}
    mass = torch.zeros(B, H, Sq, nt, dtype=torch.float64)     # log2 of the mass before tile t
    tiles_seen = torch.zeros(B, H, Sq, dtype=torch.int64)
    for t in range(nt):
        st = s[..., t * TILE:(t + 1) * TILE]
        live = okp[..., t * TILE:(t + 1) * TILE].any(-1)
        mx = st.amax(-1) * sl2
        move = mx > m + TAU
        mn = torch.where(move, mx, m)
        alpha = torch.exp2(m - mn)
        ev["rescale"][..., t] = move & seen
        ev["lazy"][..., t] = ~move & seen & (mx > m + 1.0)
        mass[..., t] = torch.log2(l.double().clamp_min(1e-300)) + m.double()
        p = torch.exp2(st * sl2 - mn[..., None])
        l = l * alpha + p.sum(-1)
        ao = alpha[..., None].expand(B, H, Sq, 128)
        if mutant == 1:
            ao = torch.cat([ao[..., :96], torch.where(seen[..., None], torch.ones(()), ao[..., 96:])], -1)
        elif mutant == 2:
            ao = torch.where(seen[..., None], alpha.index_select(axis, nb)[..., None], ao)
        O = O * ao + p.bfloat16().float() @ vv[:, :, t * TILE:(t + 1) * TILE]
        m = mn
        seen = seen | live
        tiles_seen += live
    final = torch.log2(l.double().clamp_min(1e-300)) + m.double()
    share = torch.exp2(mass - final[..., None])
    ev["relevant"] = ev["rescale"] & (share >= 0.1) & (share <= 0.9)
    return dict(out=(O / l[..., None]).bfloat16().float(), tiles_seen=tiles_seen, **ev)


def conditions(walk):
    """The input conditions of a hard case, over the rows that admit keys in at least two tiles
    (no other row can rescale after its first tile): the fractions of rows with (a) a rescale,
    (b) a lazy step, (c) a relevant rescale; and mixed: a 32-row group of one head (for a
    one-query entry: 32 heads) and a tile at which some of its rows rescale and others do not."""
    multi = walk["tiles_seen"] >= 2
    n = int(multi.sum())
    frac = {n_: float((walk[key].any(-1) & multi).sum()) / max(n, 1)
            for n_, key in (("a", "rescale"), ("b", "lazy"), ("c", "relevant"))}
    r = walk["rescale"]
    B, H, Sq, nt = r.shape
    if Sq == 1:
        r = r.reshape(B, 1, H, nt)
    mixed = False
    for g0 in range(0, r.shape[2], 32):
        grp = r[:, :, g0:g0 + 32]
        mixed |= bool((grp.any(2) & ~grp.all(2)).any())
    return dict(rows=n, all_rows=multi.numel(), mixed=mixed, **frac)


def row_err(got, ref):
    """‖got − ref‖₂ / ‖ref‖₂ over the last axis, in fp64."""
    got, ref = got.double(), ref.double()
    return (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)


@functools.lru_cache(maxsize=None)
def case_data(case, hard=True):
    """Inputs, admission mask, fp64 reference, the model's output and its worst row error: computed
    once per case, shared by every test that uses the case, never written."""
    d = make_inputs(case, hard)
    if case.entry == "probs":
        ref, model, walk = reference_probs(d["q"], d["k"]), model_probs(d["q"], d["k"]), None
    else:
        d["ok"] = admit(case)
        ref = reference(d["q"], d["k"], d["v"], d["ok"])
        walk = tile_walk(d["q"], d["k"], d["v"], d["ok"])
        model = walk["out"]
    err = row_err(model, ref)
    return dict(d, ref=ref, model=model, walk=walk, model_err=err, bound=MARGIN * float(err.max()))


def check_rows(got, case, hard=True, heads=None):
    """The criterion: every row of got (laid out as the reference, or as its listed heads) within
    MARGIN × the model's worst row.  → (worst row error, its ratio to the model's worst), for the
    record."""
    cd = case_data(case, hard)
    assert torch.isfinite(got).all(), (case.name, "non-finite output")
    err = row_err(got, cd["ref"] if heads is None else cd["ref"][:, heads])
    worst, model = float(err.max()), cd["bound"] / MARGIN
    at = tuple(int(x) for x in (err == err.max()).nonzero()[0])
    print(f"{case.name}: worst row {worst:.3e} at (b, h, row) = {at}, model {model:.3e}, ratio {worst / model:.2f}")
    assert worst <= cd["bound"], (case.name, at, worst, cd["bound"], int((err > cd["bound"]).sum()))
    return worst, worst / model


CASES = {c.name: c for c in [
    # attn_small_kernel: 1, 3 and (causal) 2 KV parts
    Case("small_1part", "attn", 1, 2, 1, 33, 65, height=460.0),
    Case("small_3parts", "attn", 2, 4, 2, 257, 641, height=20.0),
    Case("small_causal", "attn", 1, 2, 2, 257, 257, window=-2, height=24.0, profile="saw", period=150),
    # whole units, window 8
    Case("band8", "attn", 2, 4, 2, 300, 300, window=8, height=50.0, profile="saw", period=45),
    # persistent band walk
    Case("band128", "attn", 2, 4, 2, 1000, 1000, window=128, height=20.0, profile="saw", period=333, seed=2),
    Case("short_split", "attn", 1, 4, 2, 257, 641, height=20.0, seed=1),
    Case("tail_split", "attn", 2, 4, 2, 700, 1600, height=40.0),
    Case("masked_band8", "masked", 2, 2, 1, 300, 300, window=8, valid=(300, 37), height=50.0, profile="saw", period=45),
    Case("masked_full", "masked", 2, 2, 1, 1000, 1000, valid=(999, 3), height=30.0),
    Case("decode_g2", "decode", 2, 16, 8, 1, 641, height=30.0),
    Case("decode_g4", "decode", 1, 32, 8, 1, 641, height=30.0),
    Case("extend_g1", "extend", 3, 4, 4, 70, 670, pos=600, height=30.0),
    Case("extend_g2", "extend", 1, 16, 8, 70, 670, pos=600, height=30.0),
    Case("extend_g4", "extend", 1, 8, 2, 70, 670, pos=600, height=30.0),
    Case("cross_s192", "cross", 1, 4, 2, 192, 641, height=40.0),
    Case("cross_s200", "cross", 1, 4, 2, 200, 641, height=40.0),
    Case("probs", "probs", 1, 4, 2, 160, 700, height=40.0),
]}
WALK_CASES = [n for n, c in CASES.items() if c.entry != "probs"]
