#!/usr/bin/env python3
"""Bit-identity of the runtimes' outputs between two builds of the library: the check for a change
to the host code that loads the weights and drives the layers (csrc/encoder.hip, csrc/dit*.hip,
csrc/vae.hip, csrc/weights.h, csrc/abi.hip) and touches no kernel.

  --dump FILE      builds small handles with seeded weights and inputs through the public bindings
                   of the tree this script sits in, runs every entry of the encoder runtime over
                   the smallest shapes that reach each of its routes, plus one small DiT condition
                   + forward (+ forward_step) in bf16 and in the fp32 parity mode, one small VAE
                   decode + encode and one call of each stand-alone kernel entry, and saves every
                   output tensor (and the GEMM plans that show which routes ran) to FILE
  --compare A B    asserts torch.equal on the integer views of each pair of tensors of two dumps
                   and that both ran the same routes; prints one line per call

Run --dump once in a copy of each tree (each with its own library), then --compare the files.
Two dumps of one tree show first that the entries are repeatable at all.

Handles: L = 2, hidden 256, intermediate 512, head_dim 128.
  stack   full / band layers, embed (in_dim 64) and proj_out (out_dim 64), H = KV = 2, key-padding
          mask: enc_embed + enc_forward at B·S = 2·40 (the down GEMM takes the split-K path and
          leaves its residual to the next norm) and at the smallest B·S whose O and down GEMMs
          plan no split-K
  g2, g4  causal, H = 4, KV = 2 / 1, cache of 3 rows × 96: enc_forward and enc_prefill at
          B = 2, S = 37, enc_decode at pos 37 and 38, enc_extend of rows 1..2 with n = 5 at pos 39
          and n = 1 at pos 44; all of it with a left-padding mask, then without a mask
  dit     DiTConfig.tiny: Bc = 2 with the CFG row dedup and a uniform null row, set_condition,
          forward, forward_step; dit_f32: the same weights (fp32) and inputs on a parity-mode handle
  vae     VAEConfig.tiny with the encoder, fp32 weights: decode of 3 latent frames, encode (mean)
          of the decoded length
  abi     the stand-alone entries, one small call each: gemm_bf16_ex, gemm_res_norm_bf16,
          gemm_headpost_bf16, cross_attn_bf16 fused and as two launches, attention_masked_bf16,
          one APG / Euler sampler step
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ace-step-1.5_amd")]
import torch  # noqa: E402

EPI_RES = 2


def randn(g, *shape):
    return torch.randn(*shape, generator=g).bfloat16()


def dump_stack(dev, out, routes):
    from acehip import _ffi as ff
    from acehip.condition import EncoderStack
    from acehip.config import DiTConfig
    from acehip.weights import encoder_stack_shapes, synth_weights
    cfg = DiTConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                    num_key_value_heads=2, head_dim=128, sliding_window=8)

    def plans(M):   # the O and down GEMMs of this stack at M rows, as the layer loop calls them
        return {k: ff.gemm_plan(M, 256, K, EPI_RES, defer_ok=True) for k, K in (("o", 256), ("down", 512))}
    S_big = 64
    while any(p["splits"] > 1 for p in plans(2 * S_big).values()):
        S_big += 64
        assert S_big <= 16384, "no B·S without split-K found"
    st = EncoderStack(cfg, 2, 64, embed_bias=True, out_dim=64, device=0, max_tokens=2 * S_big, max_S=S_big)
    st.load(synth_weights(encoder_stack_shapes(cfg, "s", 2, 64, True, out_dim=64), 11, "parity"), prefix="s.")
    g = torch.Generator().manual_seed(5)
    for tag, S in (("small", 40), ("big", S_big)):
        x = randn(g, 2, S, 64).to(dev)
        mask = torch.ones(2, S, dtype=torch.uint8)
        mask[1, S - S // 4:] = 0                      # key padding at the end of row 1
        e = st.embed(x)
        out[f"stack.{tag}.embed"] = e
        out[f"stack.{tag}.forward"] = st.forward(e, mask.to(dev))
        routes[f"stack.{tag}"] = {"B": 2, "S": S, "plans": plans(2 * S)}
    assert routes["stack.small"]["plans"]["down"]["splits"] > 1 and routes["stack.small"]["plans"]["down"]["deferred"]
    torch.cuda.synchronize()
    st.close()


def dump_causal(dev, out, routes, name, KV):
    from acehip import _ffi as ff
    from acehip.config import DiTConfig
    from acehip.lm import HipLMRuntime
    from acehip.weights import synth_text_encoder_weights
    cfg = DiTConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                    num_key_value_heads=KV, head_dim=128)
    B, S, CAP = 2, 37, 96
    rt = HipLMRuntime(cfg, 0, max_batch=3, capacity=CAP, prefill_tokens=B * S)
    rt.load(synth_text_encoder_weights(cfg, 64, seed=13 + KV, mode="parity"))
    g = torch.Generator().manual_seed(7 + KV)
    x = randn(g, B, S, 256).to(dev)
    steps = [randn(g, B, 256).to(dev) for _ in range(2)]
    chunk, last = randn(g, B, 5, 256).to(dev), randn(g, B, 1, 256).to(dev)
    pad = torch.ones(3, CAP, dtype=torch.uint8)
    pad[1, :5] = 0                                    # left padding of sequence 1
    pad = pad.to(dev)
    for tag, km in (("mask", pad), ("nomask", None)):
        p = f"{name}.{tag}."
        out[p + "forward"] = rt.stack.forward(x, None if km is None else km[:B, :S])
        out[p + "prefill"] = rt.prefill(x, None if km is None else km[:B, :S].contiguous())
        out[p + "decode37"] = rt.decode(steps[0], km, 37)
        out[p + "decode38"] = rt.decode(steps[1], km, 38)
        out[p + "extend5"] = rt.extend(chunk, None if km is None else km[1:], 1, 39)
        out[p + "extend1"] = rt.extend(last, None if km is None else km[1:], 1, 44)
    routes[name] = {"heads": 4, "kv_heads": KV, "B": B, "S": S, "capacity": CAP,
                    "plans": {"o": ff.gemm_plan(B * S, 256, 512, EPI_RES, defer_ok=True),
                              "down": ff.gemm_plan(B * S, 256, 512, EPI_RES, defer_ok=True)}}
    torch.cuda.synchronize()
    rt.close()


def dump_dit(dev, out, routes):
    from acehip.config import DiTConfig
    from acehip.dit import DiTRuntime
    from acehip.weights import synth_dit_weights
    cfg = DiTConfig.tiny(layers=2, window=8)
    rt = DiTRuntime(cfg, 0, max_S=64, max_Bc=2, max_Lenc=32)
    rt.load({k: v.to(dev, torch.bfloat16) for k, v in synth_dit_weights(cfg, seed=1, mode="parity").items()})
    g = torch.Generator().manual_seed(3)
    xt, ctx = randn(g, 1, 47, 64).to(dev), randn(g, 1, 47, 128).to(dev)      # odd T: the crop after proj_out
    enc, null = randn(g, 1, 20, 256), randn(g, 1, 1, 256)
    rt.set_condition(torch.cat([enc, null.expand_as(enc)]).to(dev))
    rt.set_uniform_rows(1)
    t = torch.tensor([0.75], dtype=torch.float32, device=dev)
    out["dit.forward"] = rt.forward(xt, ctx, t)                               # Bx = 1, one t: the CFG row dedup
    rt.set_timesteps(torch.tensor([1.0, 0.4], device=dev))
    out["dit.forward_step"] = rt.forward_step(xt, ctx, 1)
    routes["dit"] = {"Bc": 2, "T": 47, "Lenc": 20, "uniform_from": 1}
    torch.cuda.synchronize()
    rt.close()


def dump_dit_f32(dev, out, routes):
    from acehip.config import DiTConfig
    from acehip.dit import DiTRuntime
    from acehip.weights import synth_dit_weights
    cfg = DiTConfig.tiny(layers=2, window=8)
    rt = DiTRuntime(cfg, 0, max_S=64, max_Bc=2, max_Lenc=32, dtype=torch.float32)
    rt.load({k: v.to(dev) for k, v in synth_dit_weights(cfg, seed=1, mode="parity").items()})
    g = torch.Generator().manual_seed(3)
    xt, ctx = torch.randn(1, 47, 64, generator=g).to(dev), torch.randn(1, 47, 128, generator=g).to(dev)
    rt.set_condition(torch.randn(2, 20, 256, generator=g).to(dev))
    out["dit_f32.forward"] = rt.forward(xt, ctx, torch.tensor([0.75], dtype=torch.float32, device=dev))
    routes["dit_f32"] = {"Bc": 2, "T": 47, "Lenc": 20}
    torch.cuda.synchronize()
    rt.close()


def dump_vae(dev, out, routes):
    from acehip.config import VAEConfig
    from acehip.vae import OobleckBackend
    from acehip.weights import synth_vae_weights
    cfg = VAEConfig.tiny()
    be = OobleckBackend(cfg, 0, max_T=8, with_encoder=True)
    be.load(synth_vae_weights(cfg, seed=5, mode="parity", with_encoder=True))          # fp32, from the host
    z = randn(torch.Generator().manual_seed(2), 1, 64, 3).to(dev)
    wav = be.decode_tensor(z)
    out["vae.decode"] = wav
    out["vae.encode"] = be.encode_tensor(wav, sample=False)
    routes["vae"] = {"T": 3, "hop": cfg.hop_length}
    torch.cuda.synchronize()
    be.close()


def dump_abi(dev, out, routes):
    import ctypes
    import math
    from acehip import _ffi as ff
    from acehip.dit import apg_euler_
    lib, P, sp = ff.lib(), ff.ptr, ff.stream_ptr
    g = torch.Generator().manual_seed(17)
    scale = 1.0 / math.sqrt(128.0)
    # C = A·Wᵀ on the production dispatch, then the residual GEMM whose epilogue the norm applies
    M, N, K = 40, 256, 512
    A, W = randn(g, M, K).to(dev), (0.05 * torch.randn(N, K, generator=g)).bfloat16().to(dev)
    C = torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
    ff.check(lib.acehip_gemm_bf16_ex(P(A), K, P(W), K, P(C), N, M, N, K, None, 0, -1, sp()), "gemm_ex")
    out["abi.gemm_ex"] = C
    X, w = randn(g, M, N).to(dev), (1 + 0.1 * torch.randn(N, generator=g)).bfloat16().to(dev)
    normed = torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
    deferred = ctypes.c_int(-1)
    ff.check(lib.acehip_gemm_res_norm_bf16(P(A), K, P(W), K, P(X), M, N, K, None, 0, M, 1, P(w), None, None, 0,
                                           P(normed), M, 1e-6, None, M, ctypes.byref(deferred), sp()), "gemm_res_norm")
    out["abi.gemm_res_norm.x"], out["abi.gemm_res_norm.out"] = X, normed
    # q|k|v projection with the head-post epilogue
    B, S, D, nq, nkv = 2, 40, 256, 2, 1
    xn = randn(g, B * S, D).to(dev)
    wqkv = (0.05 * torch.randn((nq + 2 * nkv) * 128, D, generator=g)).bfloat16().to(dev)
    nw = (1 + 0.1 * torch.randn(128, generator=g)).bfloat16().to(dev)
    ang = torch.arange(S)[:, None] * (1e6 ** (-torch.arange(0, 128, 2) / 128)).repeat(2)[None, :]
    cos, sin = ang.cos().bfloat16().to(dev), ang.sin().bfloat16().to(dev)
    q = torch.zeros(B, nq, S, 128, device=dev, dtype=torch.bfloat16)
    k, v = (torch.zeros(B, nkv, S, 128, device=dev, dtype=torch.bfloat16) for _ in range(2))
    ff.check(lib.acehip_gemm_headpost_bf16(P(xn), D, P(wqkv), D, B, S, nq, nkv, nkv, P(nw), P(nw), P(cos), P(sin), 1e-6,
                                           P(q), P(k), P(v), sp()), "gemm_headpost")
    out["abi.headpost.q"], out["abi.headpost.k"], out["abi.headpost.v"] = q, k, v
    # cross-attention: the fused kernel and the two launches it fuses
    B, S, H, KV, Le = 2, 200, 4, 2, 65
    xc = randn(g, B * S, D).to(dev)
    wq = (0.05 * torch.randn(H * 128, D, generator=g)).bfloat16().to(dev)
    kc, vc = randn(g, B, KV, Le, 128).to(dev), randn(g, B, KV, Le, 128).to(dev)
    paths = {}
    for force in (1, 0):
        ao = torch.zeros(B * S, H * 128, device=dev, dtype=torch.bfloat16)
        path = ctypes.c_int(-7)
        ff.check(lib.acehip_cross_attn_bf16(P(xc), P(wq), P(nw), P(kc), P(vc), P(ao), B, S, H, KV, Le, D, 1e-6, scale,
                                            force, ctypes.byref(path), sp()), "cross_attn")
        out[f"abi.cross_attn.force{force}"] = ao
        paths[f"force{force}"] = path.value
    # masked self-attention through the entry's own workspace
    B, H, S = 2, 2, 40
    qa, ka, va = (randn(g, B, H, S, 128).to(dev) for _ in range(3))
    km = torch.ones(B, S, dtype=torch.uint8)
    km[1, 30:] = 0
    km = km.to(dev)
    o = torch.zeros(B, S, H * 128, device=dev, dtype=torch.bfloat16)
    ff.check(lib.acehip_attention_masked_bf16(P(qa), P(ka), P(va), P(o), B, H, H, S, S, -1, scale, P(km), sp()), "attention")
    out["abi.attention_masked"] = o
    # one CFG + APG + Euler step
    vt, xt = randn(g, 2, 47, 64).to(dev), randn(g, 1, 47, 64).to(dev)
    ra = torch.zeros_like(xt)
    apg_euler_(vt, xt, ra, 7.0, 0.125, 1, True)
    out["abi.sampler.xt"], out["abi.sampler.ra"] = xt, ra
    routes["abi"] = {"res_norm_deferred": deferred.value, "cross_paths": paths,
                     "gemm_ex": ff.gemm_plan(M, N, K, 0), "attention": ff.attn_plan(B, H, H, S, S, -1, masked=True)}
    torch.cuda.synchronize()


def dump(path):
    from acehip import _ffi as ff
    assert torch.cuda.is_available(), "ab_enc_outputs --dump needs a GPU (no CPU path)"
    dev = torch.device("cuda:0")
    out, routes = {}, {}
    dump_stack(dev, out, routes)
    dump_causal(dev, out, routes, "g2", 2)
    dump_causal(dev, out, routes, "g4", 1)
    dump_dit(dev, out, routes)
    dump_dit_f32(dev, out, routes)
    dump_vae(dev, out, routes)
    dump_abi(dev, out, routes)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save({"build_hash": ff.build_hash(), "routes": routes, "outputs": {k: v.cpu() for k, v in out.items()}}, path)
    print(f"wrote {path}: {len(out)} tensors, build {ff.build_hash()}")
    for k, r in routes.items():
        if "plans" in r:
            print(" ", k, {n: (p["route"], p["splits"], p["deferred"]) for n, p in r["plans"].items()},
                  "(route, splits, deferred)")


def compare(a_path, b_path):
    a, b = torch.load(a_path), torch.load(b_path)
    assert a["outputs"].keys() == b["outputs"].keys(), "the dumps hold different calls"
    assert a["routes"] == b["routes"], "the dumps ran different routes"
    bad = []
    for k, ta in a["outputs"].items():
        tb = b["outputs"][k]
        bits = torch.int16 if ta.dtype == torch.bfloat16 else torch.int32
        same = ta.shape == tb.shape and ta.dtype == tb.dtype and torch.equal(ta.view(bits), tb.view(bits))
        finite = bool(torch.isfinite(ta.float()).all())
        print(f"{k:24s} {'equal' if same else 'DIFFERENT'}{'' if finite else ' (non-finite values)'}")
        if not same:
            bad.append(k)
    print(f"builds {a['build_hash']} vs {b['build_hash']}: {len(a['outputs']) - len(bad)} of {len(a['outputs'])} equal")
    assert not bad, f"outputs differ: {bad}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dump", metavar="FILE")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if bool(args.dump) == bool(args.compare):
        ap.error("give --dump FILE or --compare A B")
    if args.dump:
        dump(args.dump)
    else:
        compare(*args.compare)


if __name__ == "__main__":
    main()
