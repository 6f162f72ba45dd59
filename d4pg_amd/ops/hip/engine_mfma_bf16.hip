// bf16 MFMA GEMM kernels (v_mfma_f32_32x32x16_bf16) for the wide train step
// in gemm_precision="bf16": forward, dX and split-K dW, the bf16-operand
// twins of k_mfma_fwd / k_mfma_dx / k_mfma_dw (engine_mfma.hip).
//
// Numerics contract: both operands are fp32 in HBM and are rounded to bf16
// with round-to-nearest-even (v_cvt_pk_bf16_f32, the plain __bf16 cast) when
// they are staged into LDS; products are exact in fp32 and the MFMA
// accumulates in fp32.  Everything after the accumulator — split-K `parts`,
// bias, activation, ReLU mask, k_dw_reduce, k_head_finish — is the fp32 code
// of the f32 kernels: the C/D lane map of 32x32x16_bf16 equals that of
// 32x32x2_f32, so both call the one set of epilogues in
// engine_mfma_tile.hip.  db is the fp32 column
// sum of the bf16-rounded dz fragments the dW MFMAs consumed.  No atomics.
//
// Tile: the f32 kernels' 64x128 workgroup tile and 2x2 wave split (each wave
// 32x64 = two 32x32 accumulators), K staged in 64-deep chunks (four k-steps
// of 16), double-buffered, one barrier per chunk.  Grids, split-K factors and
// the `parts` layout are the f32 kernels' (the host computes them once); a
// split-K segment here is ceil(ceil(k/64)/ksplit) chunks, trailing segments
// may be empty and publish zeros.
//
// LDS image: both operands as [row or column of the tile][k], k fastest,
// bf16, row stride BT_LD = 72 elements (144 B): rows stay 16-byte aligned
// and the 16 rows of one ds_read_b128 lane group fall on 16 distinct 4-bank
// slots (4 * (9 r mod 16)).  Lane l reads the 8 consecutive k of row l&31 at
// k = 16 s + 8 (l>>5): one ds_read_b128 per fragment, 1.5 per MFMA.
//
// Staging, by how the operand lies in HBM:
//   k-fastest (forward X, dX dz and W): thread owns 4 consecutive k of rows
//     tid/16 + 16 u -> one float4 load and one 8-byte LDS write per row;
//   row-fastest (forward Wt, dW x and dz): the LDS write transposes — thread
//     owns 4 consecutive rows and 8 (128-row tile) or 4 (64-row tile)
//     consecutive k, loads one float4 per k and writes one 16- or 8-byte k
//     run per row.
// Tiles that are not interior, unaligned shapes and concat inputs take a
// guarded scalar load into the same registers (zero past the edge), so the
// LDS contents and the result do not depend on the path.

namespace d4pg {

#define BT_K 64
#define BT_LD 72

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// two fp32 -> two bf16 (RNE) in one dword, `lo` in the low half
__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {
    f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

__device__ __forceinline__ bool aligned16(const void* p) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

#define BF16_LDS_DECL \
    __shared__ __attribute__((aligned(16))) \
        unsigned short As2[2][MT_M * BT_LD]; \
    __shared__ __attribute__((aligned(16))) \
        unsigned short Bs2[2][MT_N * BT_LD]

// ---- LDS writers (registers -> bf16 image) ----
// k-fastest source, ROWS rows: t[4u .. 4u+3] = k kq..kq+3 of row rq + 16u
template <int ROWS>
__device__ __forceinline__ void bf16_wr_kf(unsigned short* S, const float* t,
                                           int tid) {
    const int rq = tid >> 4, kq = (tid & 15) * 4;
#pragma unroll
    for (int u = 0; u < ROWS / 16; ++u) {
        uint2 v = {pk_bf16(t[4 * u], t[4 * u + 1]),
                   pk_bf16(t[4 * u + 2], t[4 * u + 3])};
        *reinterpret_cast<uint2*>(&S[(rq + 16 * u) * BT_LD + kq]) = v;
    }
}

// row-fastest source, 128 rows: t[4u + c] = k kg + u (u < 8) of row rq + c
__device__ __forceinline__ void bf16_wr_rf128(unsigned short* S,
                                              const float* t, int tid) {
    const int rq = (tid & 31) * 4, kg = (tid >> 5) * 8;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint4 v = {pk_bf16(t[c], t[4 + c]), pk_bf16(t[8 + c], t[12 + c]),
                   pk_bf16(t[16 + c], t[20 + c]),
                   pk_bf16(t[24 + c], t[28 + c])};
        *reinterpret_cast<uint4*>(&S[(rq + c) * BT_LD + kg]) = v;
    }
}

// row-fastest source, 64 rows: t[4u + c] = k kg + u (u < 4) of row rq + c
__device__ __forceinline__ void bf16_wr_rf64(unsigned short* S,
                                             const float* t, int tid) {
    const int rq = (tid & 15) * 4, kg = (tid >> 4) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint2 v = {pk_bf16(t[c], t[4 + c]), pk_bf16(t[8 + c], t[12 + c])};
        *reinterpret_cast<uint2*>(&S[(rq + c) * BT_LD + kg]) = v;
    }
}

// The chunk loop every kernel shares.  ld(k0) loads chunk k0's A and B
// elements into the caller's registers, wr(buf) rounds them to bf16 into LDS
// buffer `buf`.  The loads of chunk ch+1 are issued before chunk ch's MFMAs
// and written to the other buffer after them; the co-resident workgroup's
// MFMAs cover the writes.  bias (wave-uniform): also sum the B fragments per
// column (the dW kernel's db) into bias0 / bias1.  Every wave of the block
// runs this one loop, so all of them meet at the same barriers.
template <typename FL, typename FW>
__device__ __forceinline__ void bf16_pipeline(FL ld, FW wr, int nch, bool bias,
                                              unsigned short (*As2)[MT_M * BT_LD],
                                              unsigned short (*Bs2)[MT_N * BT_LD],
                                              f32x16& a00, f32x16& a01,
                                              float& bias0, float& bias1) {
    if (nch <= 0) return;               // block-uniform: empty K segment
    WavePos w;
    const int wm0 = w.wm0, wn0 = w.wn0;
    int r = w.lane & 31, kh = (w.lane >> 5) * 8;
    ld(0);
    wr(0);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const unsigned short* As = As2[ch & 1];
        const unsigned short* Bs = Bs2[ch & 1];
        bool more = ch + 1 < nch;
        if (more) ld((ch + 1) * BT_K);
#pragma unroll
        for (int s = 0; s < BT_K; s += 16) {
            bf16x8 a = *reinterpret_cast<const bf16x8*>(
                &As[(wm0 + r) * BT_LD + s + kh]);
            bf16x8 b0 = *reinterpret_cast<const bf16x8*>(
                &Bs[(wn0 + r) * BT_LD + s + kh]);
            bf16x8 b1 = *reinterpret_cast<const bf16x8*>(
                &Bs[(wn0 + 32 + r) * BT_LD + s + kh]);
            a00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b0, a00, 0, 0, 0);
            a01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b1, a01, 0, 0, 0);
            if (bias) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    bias0 += (float)b0[j];
                    bias1 += (float)b1[j];
                }
            }
        }
        if (more) wr((ch + 1) & 1);
        __syncthreads();
    }
}

// C[B,out] = act(bf16(X[B,in1 (++ concat in2)]) @ bf16(Wt[in,out]) + bias);
// arguments, grid and split-K `parts` as k_mfma_fwd.
__global__ void __launch_bounds__(256, 2)
k_mfma_fwd_bf16(const float* __restrict__ x1, const float* __restrict__ x2,
                const float* __restrict__ wt, const float* __restrict__ bias,
                float* __restrict__ y, int B, int in1, int in2, int out,
                int act_kind, int ksplit, float* __restrict__ parts) {
    BF16_LDS_DECL;
    int in_total = in1 + in2;
    const MfmaTile t = mfma_tile(B, out, in_total, BT_K, ksplit);
    const int m0 = t.m0, n0 = t.n0, kbase = t.ch0 * BT_K;
    int tid = threadIdx.x;
    f32x16 acc00 = {}, acc01 = {};
    // A = X, k-fastest: rows m0 + tid/16 + 16u, k (tid%16)*4 .. +3
    // B = Wt, column-fastest: columns n0 + (tid%32)*4 .. +3, k (tid/32)*8 + u
    const int arq = tid >> 4, akq = (tid & 15) * 4;
    const int brq = (tid & 31) * 4, bkg = (tid >> 5) * 8;
    const bool vecA = (in1 % 4 == 0) && (m0 + MT_M <= B) && aligned16(x1);
    const bool vecB = (out % 4 == 0) && (n0 + MT_N <= out) && aligned16(wt);
    const GuardedCat X{x1, x2, B, in1, in2};
    const GuardedMat W{wt, in_total, out};
    float ta[16], tb[32];
    auto ld = [&](int k0r) {
        int k0 = kbase + k0r;
        mfma_stage<4>(ta, vecA && k0 + BT_K <= in1, X, [&](int u) {
            return RunPos{m0 + arq + 16 * u, k0 + akq}; });
        mfma_stage<8>(tb, vecB && k0 + BT_K <= in_total, W, [&](int u) {
            return RunPos{k0 + bkg + u, n0 + brq}; });
    };
    auto wr = [&](int buf) {
        bf16_wr_kf<MT_M>(As2[buf], ta, tid);
        bf16_wr_rf128(Bs2[buf], tb, tid);
    };
    float nb0 = 0.f, nb1 = 0.f;
    bf16_pipeline(ld, wr, t.nch, false, As2, Bs2, acc00, acc01, nb0, nb1);
    mfma_epilogue_fwd(t, acc00, acc01, bias, y, B, out, act_kind, ksplit,
                      parts);
}

// dX[B, in_lo:in_hi] = (bf16(dz[B,out]) @ bf16(Wt)^T) * act'(hprev);
// arguments and grid as k_mfma_dx.
__global__ void __launch_bounds__(256, 2)
k_mfma_dx_bf16(const float* __restrict__ dz, const float* __restrict__ wt,
               const float* __restrict__ hprev, float* __restrict__ dx,
               int B, int in_lo, int in_hi, int out, int prev_act) {
    BF16_LDS_DECL;
    int span = in_hi - in_lo;
    const MfmaTile t = mfma_tile(B, span, out, BT_K, 1, false);
    const int m0 = t.m0, n0 = t.n0;                 // n0: relative i tile
    int tid = threadIdx.x;
    f32x16 acc00 = {}, acc01 = {};
    // both operands k(=o)-fastest:
    //   A[m(=b)][k] = dz[b][o], rows m0 + tid/16 + 16u (u < 4)
    //   B[n(=i)][k] = wt[i][o], rows in_lo + n0 + tid/16 + 16u (u < 8)
    const int rq = tid >> 4, kq = (tid & 15) * 4;
    const bool vec = (out % 4 == 0) && aligned16(dz) && aligned16(wt);
    const bool vecA = vec && (m0 + MT_M <= B);
    const bool vecB = vec && (n0 + MT_N <= span);
    const GuardedMat DZ{dz, B, out};
    const GuardedMat W{wt, in_hi, out};
    float ta[16], tb[32];
    auto ld = [&](int k0) {
        bool full = k0 + BT_K <= out;
        mfma_stage<4>(ta, vecA && full, DZ, [&](int u) {
            return RunPos{m0 + rq + 16 * u, k0 + kq}; });
        mfma_stage<8>(tb, vecB && full, W, [&](int u) {
            return RunPos{in_lo + n0 + rq + 16 * u, k0 + kq}; });
    };
    auto wr = [&](int buf) {
        bf16_wr_kf<MT_M>(As2[buf], ta, tid);
        bf16_wr_kf<MT_N>(Bs2[buf], tb, tid);
    };
    float nb0 = 0.f, nb1 = 0.f;
    bf16_pipeline(ld, wr, t.nch, false, As2, Bs2, acc00, acc01, nb0, nb1);
    mfma_epilogue_dx(t, acc00, acc01, hprev, dx, B, span, prev_act);
}

// dWt[in,out] = bf16(X)^T[in,B] @ bf16(dz[B,out]) (K dimension = batch),
// db[o] = sum_b bf16(dz[b][o]); arguments, grid and split-K `parts` as
// k_mfma_dw.
__global__ void __launch_bounds__(256, 2)
k_mfma_dw_bf16(const float* __restrict__ dz, const float* __restrict__ x1,
               const float* __restrict__ x2, float* __restrict__ dwt,
               float* __restrict__ db, int B, int in1, int in2, int out,
               int ksplit, float* __restrict__ parts) {
    BF16_LDS_DECL;
    int in_total = in1 + in2;
    const MfmaTile t = mfma_tile(in_total, out, B, BT_K, ksplit);
    const int m0 = t.m0, n0 = t.n0;                 // i tile, o tile
    int b_base = t.ch0 * BT_K;
    int tid = threadIdx.x;
    f32x16 acc00 = {}, acc01 = {};
    // both operands row-fastest (k = batch row is the slow index in HBM):
    //   A[m(=i)][k(=b)] = x[b][i]: i m0 + (tid%16)*4 .. +3, b (tid/16)*4 + u
    //   B[n(=o)][k(=b)] = dz[b][o]: o n0 + (tid%32)*4 .. +3, b (tid/32)*8 + u
    const int arq = (tid & 15) * 4, akg = (tid >> 4) * 4;
    const int brq = (tid & 31) * 4, bkg = (tid >> 5) * 8;
    const bool vecA = (in1 % 4 == 0) && (m0 + MT_M <= in1) && aligned16(x1);
    const bool vecB = (out % 4 == 0) && (n0 + MT_N <= out) && aligned16(dz);
    const GuardedCat X{x1, x2, B, in1, in2};
    const GuardedMat DZ{dz, B, out};
    float ta[16], tb[32];
    auto ld = [&](int k0) {
        bool full = b_base + k0 + BT_K <= B;
        mfma_stage<4>(ta, vecA && full, X, [&](int u) {
            return RunPos{b_base + k0 + akg + u, m0 + arq}; });
        mfma_stage<8>(tb, vecB && full, DZ, [&](int u) {
            return RunPos{b_base + k0 + bkg + u, n0 + brq}; });
    };
    auto wr = [&](int buf) {
        bf16_wr_rf64(As2[buf], ta, tid);
        bf16_wr_rf128(Bs2[buf], tb, tid);
    };
    // db rides the B fragments of the wm0 == 0 waves of the m0 == 0 tiles
    // (wave-uniform choice)
    WavePos w;
    const bool want_db = db && w.wm0 == 0 && m0 == 0;
    float bias0 = 0.f, bias1 = 0.f;
    bf16_pipeline(ld, wr, t.nch, want_db, As2, Bs2, acc00, acc01, bias0,
                  bias1);
    mfma_epilogue_dw(t, acc00, acc01, bias0, bias1, want_db, dwt, db,
                     in_total, out, ksplit, parts);
}

}  // namespace d4pg
