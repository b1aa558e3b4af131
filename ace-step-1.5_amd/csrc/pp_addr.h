// pp_addr.h — where the ping-pong GEMM's LDS-DMA pieces come from, as plain integer functions:
// the kernels' two source-address sets (gemm.hip PPSrcPtr / PPSrcOff) call them, and so does the
// host-side check acehip_diag_pp_src_check, which forms every address both ways without a GPU.
//
// A wave's piece i of a K-tile is 64 lanes × 16 bytes: image row r = (wave + 8·i)·8 + lane / 8 of
// the tile's [A rows ; W rows] LDS image, 16-byte chunk (lane & 7) ^ ((image row >> 1) & 7) of
// that row's 128 bytes (the XOR swizzle, applied on the source address).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PP_HD __host__ __device__ __forceinline__
#else
#define PP_HD inline
#endif

namespace acehip {

PP_HD int pp_piece_row(int wave, int lane, int i) { return (wave + 8 * i) * 8 + (lane >> 3); }
PP_HD int pp_chunk(int lane, int image_row) { return (lane & 7) ^ ((image_row >> 1) & 7); }

// Pointer form: ELEMENT offset of the lane's piece i from A / W at K offset 0 (A rows clamp to
// M − 1; W's image rows follow the BM rows of A)
PP_HD int64_t pp_ptr_a(int M, int64_t lda, int m0, int wave, int lane, int i) {
    const int r = pp_piece_row(wave, lane, i);
    const int row = m0 + r < M - 1 ? m0 + r : M - 1;
    return (int64_t)row * lda + pp_chunk(lane, r) * 8;
}
PP_HD int64_t pp_ptr_b(int BM, int64_t ldw, int n0, int wave, int lane, int i) {
    const int r = pp_piece_row(wave, lane, i);
    return (int64_t)(n0 + r) * ldw + pp_chunk(lane, BM + r) * 8;
}

// Scalar-base form: 32-bit per-lane BYTE offsets from the tile's first A row / W row.  The
// chunk is that of piece 0 for every piece: rows 64 apart share it, and so do A and W image rows
// while BM is a multiple of 16.  Piece i of W is bstep bytes after piece 0.
PP_HD uint32_t pp_off_a(int M, int64_t lda, int m0, int wave, int lane, int i) {
    const int r0 = pp_piece_row(wave, lane, 0), last = M - 1 - m0;
    const int row = r0 + 64 * i < last ? r0 + 64 * i : last;
    return (uint32_t)row * (uint32_t)lda * 2u + (uint32_t)pp_chunk(lane, r0) * 16u;
}
PP_HD uint32_t pp_off_b(int64_t ldw, int wave, int lane) {
    const int r0 = pp_piece_row(wave, lane, 0);
    return (uint32_t)r0 * (uint32_t)ldw * 2u + (uint32_t)pp_chunk(lane, r0) * 16u;
}
PP_HD uint32_t pp_off_bstep(int64_t ldw) { return 64u * (uint32_t)ldw * 2u; }

// The scalar-base form holds what the pointer form does only while its 32-bit quantities do not
// wrap: the largest A offset (row BM − 1, chunk 7), the largest W offset (row 63) and bstep
PP_HD bool pp_saddr_fits(int BM, int64_t lda, int64_t ldw) {
    const int64_t lim = (int64_t)1 << 32;
    return lda > 0 && ldw > 0 && lda < lim && ldw < lim && (int64_t)(BM - 1) * lda * 2 + 112 < lim &&
           63 * ldw * 2 + 112 < lim && 64 * ldw * 2 < lim;
}

// ---- the K loop's LDS reads (gemm.hip pp_main) ----
// One K-tile's LDS image is BM A rows then 256 W rows of 128 bytes, XOR-swizzled by 16-byte
// chunk; the ring holds two of them, pp_buf_bytes apart.
PP_HD int pp_buf_bytes(int BM) { return (BM + 256) * 128; }
PP_HD uint32_t pp_swz(int row, int chunk) { return (uint32_t)(row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4)); }
// First A / W image row of a wave's fragments: wave group wr = wave / 4 owns BM / 2 A rows, wave
// column wc = wave % 4 owns 64 W rows.  Both are multiples of 16.
PP_HD int pp_rd_arow(int BM, int wave) { return (wave >> 2) * (BM / 2); }
PP_HD int pp_rd_brow(int BM, int wave) { return BM + (wave & 3) * 64; }
// Slot-immediate form (ACEHIP_GEMM_SLOTIMM): a lane reads row  first + 16·sub + (lane & 15),
// chunk ks·4 + lane / 16.  Rows 16 apart share their swizzle, so the address is a per-lane base —
// one per operand, k-step ks and ring slot, formed once before the K loop — plus the
// instruction's immediate 2048·sub.
PP_HD uint32_t pp_rd_base(uint32_t lds, int BM, int first_row, int lane, int ks, int slot) {
    return lds + (uint32_t)(slot * pp_buf_bytes(BM) + first_row * 128) + pp_swz(lane & 15, ks * 4 + (lane >> 4));
}
PP_HD constexpr int pp_rd_imm(int sub) { return sub * 2048; }

// EPI_CONV: the A-side K offset (elements) of K-tile k0 = tap·cin + c0 — input rows shifted by
// conv_a0 + tap·dil (negative for the front halo rows)
PP_HD int pp_conv_ko(int k0, int cin, int dil, int a0) {
    const int tap = k0 / cin;
    return k0 + tap * (dil - 1) * cin + a0 * cin;
}

}  // namespace acehip
