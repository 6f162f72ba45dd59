// f32 MFMA GEMM kernels (v_mfma_f32_32x32x2_f32 — exact fp32 at the full fp32
// rate): forward, dX and split-K dW on 64x128 workgroup tiles with double-
// buffered LDS K-slices, plus the narrow-shape helpers (k_dx_narrow,
// k_head_finish, k_dw_reduce).  Used by the wide train path (B > 512) and by
// forward-only work from 512 rows up.  Tile geometry, staging loads, the C/D
// walk and the epilogues are engine_mfma_tile.hip's, shared with the bf16
// kernels.

namespace d4pg {

// ===========================================================================
// MFMA tiled GEMM kernels (wide-batch learner path, f32-in matrix cores)
// ===========================================================================
// For the large-batch config (BASELINE config 5: B=4096, H=1024) the GEMMs
// are compute-bound and belong on the matrix cores.  gfx950's f32-in MFMA
// (v_mfma_f32_32x32x2_f32) runs at the full fp32 rate (157 TF peak) with
// EXACT f32 numerics — bitwise a k-ordered fmaf chain, i.e. the same
// summation order as the per-thread loops of the small-batch kernels.
// Tile: 64x128 per workgroup (4 waves, each 32x64 = two 32x32 MFMA tiles),
// K staged through LDS in 32-deep slices.
#define MT_K 32

#define MFMA_LDS_DECL \
    __shared__ float As2[2][MT_K * (MT_M + 4)]; \
    __shared__ float Bs2[2][MT_K * (MT_N + 4)]

__device__ __forceinline__ float4 f4(const float* t) {
    return make_float4(t[0], t[1], t[2], t[3]);
}

// The software-pipelined chunk loop of k_mfma_fwd and k_mfma_dx (k_mfma_dw
// carries its own copy, see there): double-buffered
// LDS ([k][m] and [k][n] images, rows padded by 4) — ld(k0) loads chunk k0's
// A and B elements into the caller's registers before chunk ch's MFMAs,
// wr(As, Bs) writes them to a whole buffer (the first chunk) and
// wrs(slice, Asn, Bsn) the share of MFMA slice 0..15 to the other buffer,
// one barrier per chunk.  The next chunk's LDS writes so ride the MFMA
// shadows (each kernel's wrs starts at slice 6, which trails the loads by
// ~500 MFMA-pipe cycles, past L2 latency) instead of bunching at the
// barrier, where the two co-resident workgroups' bursts convoy and expose
// the staging.
// Staging is VECTORIZED: an all-scalar staging stream (scalar loads +
// per-element bounds checks + scattered ds_writes) was ~350 VALU-pipe
// instructions per chunk — comparable to the chunk's 32 MFMAs' ~1400 MAI
// cycles — capping the H-GEMMs at ~44% of the measured 156 TF/s f32 MFMA
// peak (scripts/mfma_peak, profiles/gemm_lab).  Interior tiles load float4
// and write b128 rows where the LDS image allows, cutting staging to ~100
// instructions; edge tiles keep the guarded scalar path with bit-identical
// LDS contents.
template <typename FL, typename FW, typename FWS>
__device__ __forceinline__ void mfma_pipeline(
        FL ld, FW wr, FWS wrs, int nch,
        float (*As2)[MT_K * (MT_M + 4)], float (*Bs2)[MT_K * (MT_N + 4)],
        f32x16& a00, f32x16& a01) {
    WavePos w;
    int r = w.lane & 31, kk2 = w.lane >> 5;
    ld(0);
    wr(As2[0], Bs2[0]);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        float* As = As2[ch & 1];
        float* Bs = Bs2[ch & 1];
        float* Asn = As2[(ch + 1) & 1];
        float* Bsn = Bs2[(ch + 1) & 1];
        bool more = ch + 1 < nch;
        if (more) ld((ch + 1) * MT_K);
#pragma unroll
        for (int ks = 0; ks < MT_K; ks += 2) {
            float a0 = As[(ks + kk2) * (MT_M + 4) + w.wm0 + r];
            float b0 = Bs[(ks + kk2) * (MT_N + 4) + w.wn0 + r];
            float b1 = Bs[(ks + kk2) * (MT_N + 4) + w.wn0 + 32 + r];
            a00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, a00, 0, 0, 0);
            a01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, a01, 0, 0, 0);
            if (more) wrs(ks >> 1, Asn, Bsn);
        }
        __syncthreads();
    }
}

// C[B,out] = act(X[B,in1 (++ concat in2)] @ Wt[in,out] + bias).
// ksplit > 1: split-K over `parts` (disjoint per-segment partials summed
// by k_head_finish) — used for the narrow heads (out <= 64), whose
// M-tile-only grids (64 wgs) otherwise leave 3/4 of the chip idle.
__global__ void __launch_bounds__(256, 2)
k_mfma_fwd(const float* __restrict__ x1, const float* __restrict__ x2,
           const float* __restrict__ wt, const float* __restrict__ bias,
           float* __restrict__ y, int B, int in1, int in2, int out,
           int act_kind, int ksplit, float* __restrict__ parts) {
    MFMA_LDS_DECL;
    int in_total = in1 + in2;
    const MfmaTile t = mfma_tile(B, out, in_total, MT_K, ksplit);
    const int m0 = t.m0, n0 = t.n0, kbase = t.ch0 * MT_K;
    int tid = threadIdx.x;
    f32x16 acc00 = {}, acc01 = {};
    // staging geometry:
    //   A: thread owns row m0+tid/4, k-segment (tid%4)*8 -> 2x float4
    //      loads, scalar transposed LDS writes
    //   B: thread owns k-row tid/8, n-segment (tid%8)*16 -> 4x float4
    //      loads AND 4x b128 LDS writes (row-major, no transpose)
    const int am = tid >> 2, ak = (tid & 3) * 8;
    const int bk = tid >> 3, bn = (tid & 7) * 16;
    const bool vecA = (in1 % 4 == 0) && (m0 + MT_M <= B);
    const bool vecB = (out % 4 == 0) && (n0 + MT_N <= out);
    const GuardedCat X{x1, x2, B, in1, in2};
    const GuardedMat W{wt, in_total, out};
    float ta[8], tb[16];
    auto ld = [&](int k0r) {
        int k0 = kbase + k0r;
        mfma_stage<2>(ta, vecA && k0 + MT_K <= in1, X, [&](int u) {
            return RunPos{m0 + am, k0 + ak + 4 * u}; });
        mfma_stage<4>(tb, vecB && k0 + MT_K <= in_total, W, [&](int u) {
            return RunPos{k0 + bk, n0 + bn + 4 * u}; });
    };
    auto wr = [&](float* As, float* Bs) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
            As[(ak + u) * (MT_M + 4) + am] = ta[u];
        float4* dst = reinterpret_cast<float4*>(&Bs[bk * (MT_N + 4) + bn]);
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[u] = f4(tb + 4 * u);
    };
    // A scalar writes at slices 6..13, B b128 writes at 12..15 (the two
    // streams overlap harmlessly)
    auto wrs = [&](int sl, float* As, float* Bs) {
        if (sl >= 6 && sl < 14)
            As[(ak + sl - 6) * (MT_M + 4) + am] = ta[sl - 6];
        if (sl >= 12)
            reinterpret_cast<float4*>(
                &Bs[bk * (MT_N + 4) + bn])[sl - 12] = f4(tb + 4 * (sl - 12));
    };
    mfma_pipeline(ld, wr, wrs, t.nch, As2, Bs2, acc00, acc01);
    mfma_epilogue_fwd(t, acc00, acc01, bias, y, B, out, act_kind, ksplit,
                      parts);
}

// Narrow dX (span <= 8, the concat action slice): wave per batch row,
// lane-parallel over `out` with shfl reduce.  The MFMA path for this
// shape (one N-tile -> 64-wg grid) left 3/4 of the chip idle and its
// staging fully exposed (~76 us for 50 MFLOP); this VALU form runs the
// whole thing in ~10 us.
__global__ void k_dx_narrow(const float* __restrict__ dz,
                            const float* __restrict__ wt,
                            const float* __restrict__ ymask,
                            float* __restrict__ dx, int B, int in_lo,
                            int in_hi, int out, int prev_act) {
    int lane = threadIdx.x & 63, wrow = threadIdx.x / 64;
    int wpb = blockDim.x / 64;
    int span = in_hi - in_lo;
    for (int row = blockIdx.x * wpb + wrow; row < B;
         row += gridDim.x * wpb) {
        for (int j = 0; j < span; ++j) {
            const float* wrowp = wt + (long)(in_lo + j) * out;
            float acc = 0.f;
            for (int o = lane; o < out; o += 64)
                acc += dz[(long)row * out + o] * wrowp[o];
            for (int s = 32; s > 0; s >>= 1)
                acc += __shfl_xor(acc, s, 64);
            if (lane == 0) {
                float m_ = ymask
                    ? act_mask(prev_act, ymask[(long)row * span + j]) : 1.f;
                dx[(long)row * span + j] = acc * m_;
            }
        }
    }
}

// Head finish: y[row] = act(sum_seg parts[seg][row] + bias), wave == row
// (out <= 64); softmax reduces across the wave (softmax_wave).
__global__ void k_head_finish(const float* __restrict__ parts,
                              const float* __restrict__ bias,
                              float* __restrict__ y, int B, int out,
                              int ksplit, int act_kind) {
    int lane = threadIdx.x & 63, wrow = threadIdx.x / 64;
    int wpb = blockDim.x / 64;
    for (int row = blockIdx.x * wpb + wrow; row < B;
         row += gridDim.x * wpb) {
        float v = 0.f;
        if (lane < out) {
            for (int g = 0; g < ksplit; ++g)
                v += parts[((long)g * B + row) * out + lane];
            v += bias[lane];
        }
        if (act_kind == ACT_SOFTMAX) {
            float sm = softmax_wave(v, lane < out);
            if (lane < out) y[(long)row * out + lane] = sm;
        } else if (lane < out) {
            if (act_kind == ACT_RELU) v = fmaxf(v, 0.f);
            else if (act_kind == ACT_TANH) v = tanhf(v);
            y[(long)row * out + lane] = v;
        }
    }
}

// dX[B, in_lo:in_hi] = (dz[B,out] @ Wt^T) * act'(hprev); hprev/dx are
// [B][span] (span = in_hi - in_lo), hprev null => no mask.
__global__ void __launch_bounds__(256, 2)
k_mfma_dx(const float* __restrict__ dz, const float* __restrict__ wt,
          const float* __restrict__ hprev, float* __restrict__ dx,
          int B, int in_lo, int in_hi, int out, int prev_act) {
    MFMA_LDS_DECL;
    int span = in_hi - in_lo;
    const MfmaTile t = mfma_tile(B, span, out, MT_K, 1, false);
    const int m0 = t.m0, n0 = t.n0;                 // n0: relative i tile
    int tid = threadIdx.x;
    f32x16 acc00 = {}, acc01 = {};
    // staging geometry:
    //   A[k(=o)][m(=b)] = dz[b][o]: thread owns dz-row m0+tid/4,
    //     o-segment (tid%4)*8 -> 2x float4 loads, scalar transposed
    //     LDS writes
    //   B[k(=o)][n(=i)] = wt[i][o]: thread owns wt-row in_lo+n0+tid/2,
    //     o-segment (tid%2)*16 -> 4x float4 loads, scalar transposed
    //     LDS writes
    const int am = tid >> 2, ak = (tid & 3) * 8;
    const int bnn = tid >> 1, bkk = (tid & 1) * 16;
    const bool vecA = (out % 4 == 0) && (m0 + MT_M <= B);
    const bool vecB = (out % 4 == 0) && (n0 + MT_N <= span);
    const GuardedMat DZ{dz, B, out};
    const GuardedMat W{wt, in_hi, out};
    float ta[8], tb[16];
    auto ld = [&](int k0) {
        bool full = k0 + MT_K <= out;
        mfma_stage<2>(ta, vecA && full, DZ, [&](int u) {
            return RunPos{m0 + am, k0 + ak + 4 * u}; });
        mfma_stage<4>(tb, vecB && full, W, [&](int u) {
            return RunPos{in_lo + n0 + bnn, k0 + bkk + 4 * u}; });
    };
    auto wr = [&](float* As, float* Bs) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
            As[(ak + u) * (MT_M + 4) + am] = ta[u];
#pragma unroll
        for (int u = 0; u < 16; ++u)
            Bs[(bkk + u) * (MT_N + 4) + bnn] = tb[u];
    };
    // one A element + two B elements per slice over slices 6..13
    auto wrs = [&](int sl, float* As, float* Bs) {
        if (sl >= 6 && sl < 14) {
            int u = sl - 6;
            As[(ak + u) * (MT_M + 4) + am] = ta[u];
            Bs[(bkk + 2 * u) * (MT_N + 4) + bnn] = tb[2 * u];
            Bs[(bkk + 2 * u + 1) * (MT_N + 4) + bnn] = tb[2 * u + 1];
        }
    };
    mfma_pipeline(ld, wr, wrs, t.nch, As2, Bs2, acc00, acc01);
    mfma_epilogue_dx(t, acc00, acc01, hprev, dx, B, span, prev_act);
}

// Split-K partial reduce: dwt[i,o] = sum_seg parts[seg][i,o] (+ db tail).
// Replaces the fp32-atomicAdd epilogue of the split-K dW: 2.1M atomics per
// H-layer dW cost ~80 us of L2 read-modify-write serialization, while
// disjoint partials + this bandwidth-bound sweep cost ~3 us
// (profiles/gemm_lab evidence).
__global__ void k_dw_reduce(const float* __restrict__ parts,
                            float* __restrict__ dwt, float* __restrict__ db,
                            long nw, int out, int ksplit) {
    long total = nw + (db ? out : 0);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long)gridDim.x * blockDim.x) {
        float s = 0.f;
        if (i < nw) {
            for (int g = 0; g < ksplit; ++g)
                s += parts[(long)g * nw + i];
            dwt[i] = s;
        } else {
            long j = i - nw;
            for (int g = 0; g < ksplit; ++g)
                s += parts[(long)ksplit * nw + (long)g * out + j];
            db[j] = s;
        }
    }
}

// dWt[in,out] = X^T[in,B] @ dz[B,out]  (K dimension = batch).  Split-K
// over `ksplit` segments (grid = nti*nto*ksplit): with ksplit > 1 every
// segment stores its own partials in `parts` and k_dw_reduce sums them, with
// ksplit == 1 the tile is stored to dwt directly; no atomics, nothing to
// pre-zero.  The bias db[o] = sum_b dz[b][o] accumulates for free out of the
// B fragments during the MFMA loop (wm0 == 0 waves of the m0 == 0 tiles).
// This kernel keeps its own loaders and its own copy of the chunk loop (A
// b128 writes at slices 6 and 7, B at 8..11): built on mfma_stage and
// mfma_pipeline it computed the same bits but ran 11% slower on the MI355X
// (63.4 against 57.2 us at B=4096, H=1024; NOTES.md), so only its tile
// geometry and its epilogue are the shared ones.
__global__ void __launch_bounds__(256, 2)
k_mfma_dw(const float* __restrict__ dz, const float* __restrict__ x1,
          const float* __restrict__ x2, float* __restrict__ dwt,
          float* __restrict__ db, int B, int in1, int in2, int out,
          int ksplit, float* __restrict__ parts) {
    MFMA_LDS_DECL;
    int in_total = in1 + in2;
    const MfmaTile t = mfma_tile(in_total, out, B, MT_K, ksplit);
    const int m0 = t.m0, n0 = t.n0;                 // i tile, o tile
    const int nch = t.nch;
    long b_base = (long)t.ch0 * MT_K;
    int tid = threadIdx.x, lane = tid & 63;
    f32x16 acc00 = {}, acc01 = {};
    // Vectorized staging (same rationale as k_mfma_fwd):
    //   A[k(=b)][m(=i)]: thread owns batch-row b_base+k0+tid/8,
    //     i-segment (tid%8)*8 -> 2x float4 loads AND b128 LDS writes
    //     (no transpose: global and LDS are both i-fastest)
    //   B[k(=b)][n(=o)]: thread owns batch-row tid/8, o-segment
    //     (tid%8)*16 -> 4x float4 loads and b128 writes
    const int akb = tid >> 3, ai = (tid & 7) * 8;
    const int bo = (tid & 7) * 16;
    const bool vecA = (in1 % 4 == 0) && (m0 + MT_M <= in1);
    const bool vecB = (out % 4 == 0) && (n0 + MT_N <= out);
    float4 ta[2], tb[4];
    auto ldA = [&](int k0) {
        long gb = b_base + k0 + akb;
        if (vecA && b_base + k0 + MT_K <= B) {
            const float* src = x1 + gb * in1 + m0 + ai;
            ta[0] = *reinterpret_cast<const float4*>(src);
            ta[1] = *reinterpret_cast<const float4*>(src + 4);
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int gi = m0 + ai + u;
                float v = 0.f;
                if (gb < B && gi < in_total)
                    v = (gi < in1) ? x1[gb * in1 + gi]
                                   : x2[gb * in2 + (gi - in1)];
                reinterpret_cast<float*>(ta)[u] = v;
            }
        }
    };
    auto ldB = [&](int k0) {
        long gb = b_base + k0 + akb;
        if (vecB && b_base + k0 + MT_K <= B) {
            const float4* src =
                reinterpret_cast<const float4*>(dz + gb * out + n0 + bo);
#pragma unroll
            for (int u = 0; u < 4; ++u) tb[u] = src[u];
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                int go = n0 + bo + u;
                reinterpret_cast<float*>(tb)[u] =
                    (gb < B && go < out) ? dz[gb * out + go] : 0.f;
            }
        }
    };
    float bias0 = 0.f, bias1 = 0.f;
    {
        int wid = tid >> 6;
        int wm0 = (wid >> 1) * 32, wn0 = (wid & 1) * 64;
        int r = lane & 31, kk2 = lane >> 5;
        ldA(0);
        ldB(0);
        auto wr = [&](float* As, float* Bs) {
            float4* da =
                reinterpret_cast<float4*>(&As[akb * (MT_M + 4) + ai]);
            da[0] = ta[0];
            da[1] = ta[1];
            float4* dbp =
                reinterpret_cast<float4*>(&Bs[akb * (MT_N + 4) + bo]);
#pragma unroll
            for (int u = 0; u < 4; ++u) dbp[u] = tb[u];
        };
        wr(As2[0], Bs2[0]);
        __syncthreads();
        for (int ch = 0; ch < nch; ++ch) {
            float* As = As2[ch & 1];
            float* Bs = Bs2[ch & 1];
            float* Asn = As2[(ch + 1) & 1];
            float* Bsn = Bs2[(ch + 1) & 1];
            bool more = ch + 1 < nch;
            if (more) {
                ldA((ch + 1) * MT_K);
                ldB((ch + 1) * MT_K);
            }
#pragma unroll
            for (int ks = 0; ks < MT_K; ks += 2) {
                float a0 = As[(ks + kk2) * (MT_M + 4) + wm0 + r];
                float b0 = Bs[(ks + kk2) * (MT_N + 4) + wn0 + r];
                float b1 = Bs[(ks + kk2) * (MT_N + 4) + wn0 + 32 + r];
                acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
                acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
                if (wm0 == 0) { bias0 += b0; bias1 += b1; }
                // next chunk's LDS writes ride the MFMA shadows
                if (more) {
                    int sl = ks >> 1;
                    if (sl == 6)
                        reinterpret_cast<float4*>(
                            &Asn[akb * (MT_M + 4) + ai])[0] = ta[0];
                    else if (sl == 7)
                        reinterpret_cast<float4*>(
                            &Asn[akb * (MT_M + 4) + ai])[1] = ta[1];
                    else if (sl >= 8 && sl < 12)
                        reinterpret_cast<float4*>(
                            &Bsn[akb * (MT_N + 4) + bo])[sl - 8] = tb[sl - 8];
                }
            }
            __syncthreads();
        }
    }
    WavePos w;
    mfma_epilogue_dw(t, acc00, acc01, bias0, bias1,
                     db && w.wm0 == 0 && m0 == 0, dwt, db, in_total, out,
                     ksplit, parts);
}

}  // namespace d4pg
