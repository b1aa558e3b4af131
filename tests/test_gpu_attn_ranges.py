"""Every attention route on inputs whose scores span tens of nats along the key axis, so that the
online softmax's reference max really moves: O and l are rescaled by alpha ≠ 1 with a non-empty
accumulator, P reaches 2⁸ inside the lazy region, partials with different maxima are merged, and
one wave holds rows that rescale at a tile beside rows that do not.  The randn inputs of the other
attention tests never do any of this (tests/test_attn_ranges_host.py shows it on the CPU).

Inputs, fp64 reference, the tile-walk model and the criterion are tests/attn_range_ref.py's: per
(batch, head, query row) ‖got − ref‖₂ / ‖ref‖₂ over the row's 128 outputs (for the probabilities
entry: over the row's keys), every row within 2 × the model's worst row on the same inputs.  The
bound comes from the model at run time, never from the kernel.  Each route asserts its plan before
the launch (acehip_diag_attn_plan / acehip_diag_attn_extend_plan; acehip_attention_decode_bf16 has
no plan query: its arms are the ones tests/test_gpu_attn_decode.py runs).  Routes that the other
tests launch three times for bit-reproducibility do so here: the part order of a merge matters
when the maxima differ.

Measured on an MI355X: the kernel's worst row error, and its ratio to the model's worst row.
  attn_small_kernel           1 part 2.62e-3 (0.75); 3 parts 2.87e-3 (0.74); causal, 2 parts 2.72e-3 (0.80)
  whole units, window 8       attn_fwd_kernel<2> 4.11e-3 (1.00); attn_pw_kernel 4.11e-3 (1.00)
  persistent band walk        attn_pw_kernel 4.03e-3 (1.00), bit-equal to one workgroup per unit
  short split                 4 parts 2.92e-3 (0.92), 2 parts 3.19e-3 (1.00), on either kernel
  tail split, stream-K        3.67e-3 (1.00) in all six arms
  key padding                 window 8 3.35e-3 (1.00); attn_small_kernel 3.53e-3 (0.96); 6-part split 3.02e-3 (0.82)
  attention_decode            G = 2 1.83e-3 (0.68), G = 4 1.98e-3 (0.66), with and without parts (fp32 P)
  attention_extend            one part 3.84e-3 / 3.89e-3 / 3.27e-3 (1.00 each, G = 1 / 2 / 4); 6 parts
                              3.84e-3 (1.00) / 3.45e-3 (0.89) / 3.75e-3 (1.15); 4 parts, G = 4 4.28e-3 (1.31)
  cross_attn                  3.93e-3 (1.00), fused and two launches, S 192 and 200
  attention_probs             3.04e-3 (1.00)
A ratio of 1.00 is the same worst row with the same error to four digits: on a one-range route the
model reproduces the kernel's roundings.  No route exceeded the bound; no kernel was changed.
The host test's mutants, on the same inputs: worst row 0.5 .. 8e2, 17 .. 5600 rows over the bound
per case; on the randn inputs of the same seeds neither mutant changes a single output."""
import ctypes

import pytest
import torch

import attn_range_ref as R
from conftest import set_knob

pytestmark = pytest.mark.gpu

SCALE = R.SCALE
CAP = 704                       # decode / extend cache rows: 641 and 670 valid ones, NaN behind them
_dev = {}


def _ff():
    from acehip import _ffi
    return _ffi


def _inputs(name, dev):
    """The case's bf16 inputs on the GPU (made once, never written)."""
    if name not in _dev:
        d = R.case_data(R.CASES[name])
        _dev[name] = {k: d[k].to(dev).contiguous() for k in ("q", "k", "v", "xn", "wq", "qnw") if k in d}
    return _dev[name]


def _rows(o, B, H, S):
    """token-major [B·S][H·128] → [B, H, S, 128] fp32 on the CPU."""
    return o.float().cpu().view(B, S, H, 128).permute(0, 2, 1, 3)


def _attention(name, dev, launches=1, kmask=None):
    """acehip_attention_bf16 / acehip_attention_masked_bf16 on a case, `launches` times into
    NaN-filled outputs, all bit-equal → [B, H, Sq, 128]."""
    ff, c, d = _ff(), R.CASES[name], _inputs(name, dev)
    outs = []
    for _ in range(launches):
        o = torch.full((c.B, c.Sq, c.H * 128), float("nan"), device=dev, dtype=torch.bfloat16)
        if kmask is None:
            rc = ff.lib().acehip_attention_bf16(ff.ptr(d["q"]), ff.ptr(d["k"]), ff.ptr(d["v"]), ff.ptr(o), c.B, c.H,
                                                c.KV, c.Sq, c.Sk, c.window, SCALE, ff.stream_ptr())
        else:
            rc = ff.lib().acehip_attention_masked_bf16(ff.ptr(d["q"]), ff.ptr(d["k"]), ff.ptr(d["v"]), ff.ptr(o), c.B,
                                                       c.H, c.KV, c.Sq, c.Sk, c.window, SCALE, ff.ptr(kmask),
                                                       ff.stream_ptr())
        ff.check(rc, name)
        torch.cuda.synchronize()
        outs.append(o)
    for o in outs[1:]:
        assert torch.equal(outs[0].view(torch.int16), o.view(torch.int16)), (name, "launches differ")
    return _rows(outs[0], c.B, c.H, c.Sq)


def _plan(name, masked=False, **want):
    c = R.CASES[name]
    plan = _ff().attn_plan(c.B, c.H, c.KV, c.Sq, c.Sk, c.window, masked=masked)
    assert {k: plan[k] for k in want} == want, (name, plan)


@pytest.mark.parametrize("name,units,parts,causal", [("small_1part", 4, 1, 0), ("small_3parts", 72, 3, 0),
                                                     ("small_causal", 18, 2, 1)])
def test_small_kernel(gpu_device, name, units, parts, causal):
    """attn_small_kernel: the four waves' LDS fold and the part fold through the workspace."""
    ff = _ff()
    _plan(name, kernel=ff.ATTN_SMALL, units=units, parts=parts, causal=causal, uses_ws=int(parts > 1))
    R.check_rows(_attention(name, gpu_device, launches=3), R.CASES[name])


@pytest.mark.parametrize("pw", ["0", "7"])
def test_whole_units_window_8(gpu_device, monkeypatch, pw):
    """attn_fwd_kernel<2> ("0") and attn_pw_kernel ("7"), one workgroup per unit, three tiles."""
    ff = _ff()
    set_knob(monkeypatch, "ACEHIP_ATTN_PW", pw)
    _plan("band8", kernel=ff.ATTN_PW if pw == "7" else ff.ATTN_FWD, nrep=2, units=12, unit_tiles=3, nsplit=1, persist=0,
          streamk=0, grid=12)
    R.check_rows(_attention("band8", gpu_device), R.CASES["band8"])


def test_band_persistent_walk(gpu_device, monkeypatch):
    """attn_pw_kernel walking two units per workgroup (pw_oscale on every rescale), bit-equal to
    one workgroup per unit."""
    ff = _ff()
    set_knob(monkeypatch, "ACEHIP_ATTN_CUS", "16")
    outs = {}
    for pers in ("1", "0"):
        set_knob(monkeypatch, "ACEHIP_ATTN_PERSIST", pers)
        _plan("band128", kernel=ff.ATTN_PW, units=32, unit_tiles=7, nsplit=1, persist=int(pers),
              grid=16 if pers == "1" else 32)
        outs[pers] = _attention("band128", gpu_device)
    R.check_rows(outs["1"], R.CASES["band128"])
    assert torch.equal(outs["1"], outs["0"])


@pytest.mark.parametrize("pw,cus", [("0", 0), ("0", 16), ("7", 0), ("7", 16)])
def test_short_split(gpu_device, monkeypatch, pw, cus):
    """Every unit as 4 (2 on 16 CUs) KV-range parts, merged by slab_fold in part order."""
    ff = _ff()
    set_knob(monkeypatch, "ACEHIP_ATTN_SMALL", "0")
    set_knob(monkeypatch, "ACEHIP_ATTN_PW", pw)
    if cus:
        set_knob(monkeypatch, "ACEHIP_ATTN_CUS", str(cus))
    nsplit = 2 if cus else 4
    _plan("short_split", kernel=ff.ATTN_PW if pw == "7" else ff.ATTN_FWD, nrep=2, units=6, unit_tiles=11, full=0,
          nsplit=nsplit, grid=6 * nsplit, streamk=0, uses_ws=1)
    R.check_rows(_attention("short_split", gpu_device, launches=3), R.CASES["short_split"])


@pytest.mark.parametrize("arm", ["pw", "streamk", "fwd_split"])
@pytest.mark.parametrize("cus", [16, 20])
def test_tail_split_and_streamk(gpu_device, monkeypatch, cus, arm):
    """24 units of 25 tiles on 16 / 20 CUs: the tail's 2- / 4-way split on attn_pw_kernel and (stream-K
    off) on attn_fwd_kernel<2>, and the stream-K hand-off that is attn_fwd_kernel<2>'s default."""
    ff = _ff()
    set_knob(monkeypatch, "ACEHIP_ATTN_CUS", str(cus))
    set_knob(monkeypatch, "ACEHIP_ATTN_PW", "7" if arm == "pw" else "0")
    if arm == "fwd_split":
        set_knob(monkeypatch, "ACEHIP_ATTN_STREAMK", "0")
    if arm == "streamk":
        _plan("tail_split", kernel=ff.ATTN_FWD, nrep=2, units=24, unit_tiles=25, streamk=1, sk_nt=25, sk_total=600,
              grid=cus, uses_ws=1)
    else:
        _plan("tail_split", kernel=ff.ATTN_PW if arm == "pw" else ff.ATTN_FWD, nrep=2, units=24, unit_tiles=25,
              full=cus, nsplit={16: 2, 20: 4}[cus], streamk=0, uses_ws=1)
    R.check_rows(_attention("tail_split", gpu_device, launches=3), R.CASES["tail_split"])


def _kmask(name, dev):
    c = R.CASES[name]
    m = torch.zeros(c.B, c.Sk, dtype=torch.uint8)
    for b, n in enumerate(c.valid):
        m[b, :n] = 1
    return m.to(dev)


def test_key_padding_window_8(gpu_device):
    """attn_fwd_kernel's masked mode (every tile visited; batch row 1 keeps 37 keys, so its rows
    past 45 admit none and weigh all keys uniformly, as the entry documents)."""
    ff = _ff()
    _plan("masked_band8", masked=True, kernel=ff.ATTN_FWD, nrep=2, units=6, unit_tiles=5, nsplit=1, streamk=0, grid=6)
    R.check_rows(_attention("masked_band8", gpu_device, kmask=_kmask("masked_band8", gpu_device)),
                 R.CASES["masked_band8"])


@pytest.mark.parametrize("mode", ["1", "0"])
def test_key_padding_full(gpu_device, monkeypatch, mode):
    """attn_small_kernel's key-padding mode, 2 parts ("1"), and attn_fwd_kernel's as a 6-part short
    split ("0")."""
    ff = _ff()
    set_knob(monkeypatch, "ACEHIP_ATTN_SMALL_MASK", mode)
    if mode == "1":
        _plan("masked_full", masked=True, kernel=ff.ATTN_SMALL, units=128, parts=2, uses_ws=1)
    else:
        _plan("masked_full", masked=True, kernel=ff.ATTN_FWD, nrep=2, units=16, unit_tiles=16, full=0, nsplit=6,
              streamk=0, uses_ws=1)
    R.check_rows(_attention("masked_full", gpu_device, launches=3, kmask=_kmask("masked_full", gpu_device)),
                 R.CASES["masked_full"])


def _cache(t, dev):
    """[B, KV, n, 128] → a [B, KV, CAP, 128] cache whose rows past n hold NaN."""
    B, KV, n, _ = t.shape
    c = torch.full((B, KV, CAP, 128), float("nan"), device=dev, dtype=torch.bfloat16)
    c[:, :, :n] = t
    return c


@pytest.mark.parametrize("ws,cus", [(False, 0), (True, 4), (True, 24)])
@pytest.mark.parametrize("name", ["decode_g2", "decode_g4"])
def test_decode(gpu_device, monkeypatch, name, ws, cus):
    """acehip_attention_decode_bf16, n = 641 of 704 cache rows: one key range per KV head (no
    workspace) and the part counts of 4 and 24 planned CUs through attn_decode_fold_kernel."""
    ff, c, d = _ff(), R.CASES[name], _inputs(name, gpu_device)
    if cus:
        set_knob(monkeypatch, "ACEHIP_ATTN_CUS", str(cus))
    q = d["q"].reshape(c.B, c.H, 128)
    k, v = _cache(d["k"], gpu_device), _cache(d["v"], gpu_device)
    nb = ff.lib().acehip_attention_decode_ws_bytes(c.B, c.H) if ws else 0
    outs = []
    for _ in range(2):
        wsb = torch.full((nb // 4,), float("nan"), device=gpu_device, dtype=torch.float32) if ws else None
        o = torch.full((c.B, c.H * 128), float("nan"), device=gpu_device, dtype=torch.bfloat16)
        ff.check(ff.lib().acehip_attention_decode_bf16(ff.ptr(q), ff.ptr(k), ff.ptr(v), ff.ptr(o), c.B, c.H, c.KV, c.Sk,
                                                       CAP, None, 0, SCALE, ff.ptr(wsb), nb, ff.stream_ptr()), name)
        torch.cuda.synchronize()
        outs.append(o)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    R.check_rows(outs[0].float().cpu().view(c.B, c.H, 1, 128), c)


# key-range parts of n = 70 at pos = 600 (11 tiles) by ACEHIP_ATTN_CUS (0: the device's 256)
_EXTEND_PARTS = {"extend_g1": {0: 6, 4: 1, 24: 2}, "extend_g2": {0: 6, 4: 1, 24: 1}, "extend_g4": {0: 6, 4: 1, 24: 4}}


@pytest.mark.parametrize("cus", [0, 4, 24])
@pytest.mark.parametrize("name", list(_EXTEND_PARTS))
def test_extend(gpu_device, monkeypatch, name, cus):
    """acehip_attention_extend_bf16, 70 queries at cache positions 600..669 (query i admits keys
    ≤ 600 + i), H / KV = 1, 2 and 4: whole units and 2 to 6 key ranges folded in part order."""
    ff, c, d = _ff(), R.CASES[name], _inputs(name, gpu_device)
    if cus:
        set_knob(monkeypatch, "ACEHIP_ATTN_CUS", str(cus))
    parts = _EXTEND_PARTS[name][cus]
    p = ff.attn_extend_plan(c.B, c.H, c.KV, c.Sq, c.pos)
    assert (p["tiles"], p["parts"], p["uses_ws"]) == (11, parts, int(parts > 1)), p
    k, v = _cache(d["k"], gpu_device), _cache(d["v"], gpu_device)
    nb = ff.lib().acehip_attention_extend_ws_bytes(c.B, c.H, c.Sq)
    outs = []
    for _ in range(2):
        ws = torch.full((nb // 4,), float("nan"), device=gpu_device, dtype=torch.float32)
        o = torch.full((c.B * c.Sq, c.H * 128), float("nan"), device=gpu_device, dtype=torch.bfloat16)
        ff.check(ff.lib().acehip_attention_extend_bf16(ff.ptr(d["q"]), ff.ptr(k), ff.ptr(v), ff.ptr(o), c.B, c.H, c.KV,
                                                       c.Sq, c.pos, CAP, None, 0, SCALE, ff.ptr(ws), nb,
                                                       ff.stream_ptr()), name)
        torch.cuda.synchronize()
        outs.append(o)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    R.check_rows(_rows(outs[0], c.B, c.H, c.Sq), c)


@pytest.mark.parametrize("name", ["cross_s192", "cross_s200"])
def test_cross_fused_and_two_launches(gpu_device, name):
    """acehip_cross_attn_bf16 forced to the fused kernel (1) and to projection + attn_fwd_kernel<2>
    (0), 641 cached keys: each against fp64 on the q that the head-post epilogue writes
    (attn_range_ref.cross_q), and bit-equal to each other."""
    ff, c, d = _ff(), R.CASES[name], _inputs(name, gpu_device)
    outs = {}
    for force in (0, 1):
        ao = torch.full((c.B * c.Sq, c.H * 128), float("nan"), device=gpu_device, dtype=torch.bfloat16)
        path = ctypes.c_int(-7)
        ff.check(ff.lib().acehip_cross_attn_bf16(ff.ptr(d["xn"]), ff.ptr(d["wq"]), ff.ptr(d["qnw"]), ff.ptr(d["k"]),
                                                 ff.ptr(d["v"]), ff.ptr(ao), c.B, c.Sq, c.H, c.KV, c.Sk, R.CROSS_D,
                                                 R.CROSS_EPS, SCALE, force, ctypes.byref(path), ff.stream_ptr()), name)
        torch.cuda.synchronize()
        assert path.value == force
        outs[force] = ao
        R.check_rows(_rows(ao, c.B, c.H, c.Sq), c)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


def test_probs_full_key_range(gpu_device):
    """acehip_attention_probs_bf16, every head, all 700 keys: per query row over the keys."""
    ff, c, d = _ff(), R.CASES["probs"], _inputs("probs", gpu_device)
    heads = [3, 0, 2, 1]
    hs = (ctypes.c_int * len(heads))(*heads)
    out = torch.full((len(heads), c.B, c.Sk, c.Sq), float("nan"), device=gpu_device, dtype=torch.float32)
    ff.check(ff.lib().acehip_attention_probs_bf16(ff.ptr(d["q"]), ff.ptr(d["k"]), c.B, c.H, c.KV, c.Sq, c.Sk, hs,
                                                  len(heads), 0, c.Sk, SCALE, ff.ptr(out), ff.stream_ptr()), "probs")
    torch.cuda.synchronize()
    R.check_rows(out.cpu().permute(1, 0, 3, 2), c, heads=heads)
