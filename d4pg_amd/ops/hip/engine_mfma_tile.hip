// What the f32 (engine_mfma.hip) and bf16 (engine_mfma_bf16.hip) MFMA GEMM
// kernels share: the 64x128 workgroup tile and its split-K geometry, the
// staging loader, the C/D lane map and the three epilogues.  Both MFMA shapes
// (32x32x2_f32, 32x32x16_bf16) leave the accumulator in the same lanes and
// registers, so everything after the chunk loop is one fp32 text.

namespace d4pg {

// Workgroup tile: 4 waves as 2x2, each 32x64 = two 32x32 accumulators.
// M-tile 64 (not 128): the H=1024 layers' grids then cover the chip with
// 2 workgroups per CU, so one workgroup's LDS staging hides behind the
// other's MFMAs (at 128 the 256-wg grid left 1 wg/CU and the per-chunk
// ds_write+barrier was exposed — ~50% MfmaUtil).
#define MT_M 64
#define MT_N 128

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- tile geometry ----
// Grid = ksplit segments x (row tiles x column tiles), column tile fastest.
// The K extent is cut into chunks of `kdepth`; segment `seg` owns the `nch`
// chunks from `ch0` on (ceil split).
// nch <= 0: an empty tail segment (a chunk count that is no multiple of
// ksplit, e.g. B=640: 20 chunks of 32 over 16 segments).  It must still
// publish ZERO partials — k_dw_reduce / k_head_finish sum all ksplit segments
// and `parts` holds stale data from earlier GEMMs — so the kernels run their
// epilogue on the zero accumulator; every load of such a segment is past the
// K extent and so guarded to zero.
struct MfmaTile { int seg, m0, n0, ch0, nch; };

// split = false (a literal, dX): the grid is the tiles alone, one segment.
__device__ __forceinline__ MfmaTile mfma_tile(int rows, int cols, int kext,
                                              int kdepth, int ksplit,
                                              bool split = true) {
    int ntn = (cols + MT_N - 1) / MT_N;
    int nt = ((rows + MT_M - 1) / MT_M) * ntn;
    MfmaTile t;
    t.seg = split ? blockIdx.x / nt : 0;
    int tile = split ? blockIdx.x % nt : blockIdx.x;
    t.m0 = (tile / ntn) * MT_M;
    t.n0 = (tile % ntn) * MT_N;
    int nch_total = (kext + kdepth - 1) / kdepth;
    int nch_seg = (nch_total + ksplit - 1) / ksplit;
    t.ch0 = t.seg * nch_seg;
    t.nch = min(nch_seg, nch_total - t.ch0);
    return t;
}

// ---- staging loads ----
// A staged operand is a row-major fp32 matrix (or the concat [x1 | x2]) read
// in runs of 4 consecutive columns.  at(r, c) is the unguarded address, for
// interior aligned runs; (r, c) the guarded element, zero past the edge, so
// the registers — and the LDS image — do not depend on the path.
struct GuardedMat {
    const float* p;
    int rows, cols;
    __device__ __forceinline__ const float* at(int r, int c) const {
        return p + (long)r * cols + c;
    }
    __device__ __forceinline__ float operator()(int r, int c) const {
        return (r < rows && c < cols) ? p[(long)r * cols + c] : 0.f;
    }
};

struct GuardedCat {                 // [x1 (in1 columns) | x2 (in2 columns)]
    const float *x1, *x2;
    int rows, in1, in2;
    __device__ __forceinline__ const float* at(int r, int c) const {
        return x1 + (long)r * in1 + c;          // runs inside x1 only
    }
    __device__ __forceinline__ float operator()(int r, int c) const {
        float v = 0.f;
        if (r < rows && c < in1 + in2)
            v = (c < in1) ? x1[(long)r * in1 + c]
                          : x2[(long)r * in2 + (c - in1)];
        return v;
    }
};

struct RunPos { int r, c; };

// t[4u .. 4u+3] = the run of 4 at pos(u), u < N: one float4 load each when
// `vec` (the caller has checked interior, row length % 4 and base alignment),
// else guarded scalars into the same registers.
template <int N, typename M, typename FP>
__device__ __forceinline__ void mfma_stage(float* t, bool vec, const M& mat,
                                           FP pos) {
    if (vec) {
#pragma unroll
        for (int u = 0; u < N; ++u) {
            auto p = pos(u);
            float4 v = *reinterpret_cast<const float4*>(mat.at(p.r, p.c));
            t[4 * u] = v.x; t[4 * u + 1] = v.y;
            t[4 * u + 2] = v.z; t[4 * u + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int u = 0; u < N; ++u) {
            auto p = pos(u);
#pragma unroll
            for (int c = 0; c < 4; ++c) t[4 * u + c] = mat(p.r, p.c + c);
        }
    }
}

// ---- the C/D walk ----
// The lane map of a 32x32 accumulator: register `reg` of lane `lane` is
// row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), column lane & 31.  Visits the
// wave's 2 x 16 registers and hands f(tile row, tile column, value).
struct WavePos {
    int lane, wm0, wn0;             // wave origin inside the workgroup tile
    __device__ __forceinline__ WavePos() {
        int wid = threadIdx.x >> 6;
        lane = threadIdx.x & 63;
        wm0 = (wid >> 1) * 32;
        wn0 = (wid & 1) * 64;
    }
};

template <typename F>
__device__ __forceinline__ void mfma_cd_walk(const f32x16& a00,
                                             const f32x16& a01, F f) {
    WavePos w;
    const f32x16* accs[2] = {&a00, &a01};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            int row = (reg & 3) + 8 * (reg >> 2) + 4 * (w.lane >> 5);
            f(w.wm0 + row, w.wn0 + t * 32 + (w.lane & 31), (*accs[t])[reg]);
        }
    }
}

// ---- epilogues ----
// forward: split-K partials (k_head_finish sums and finishes) or
// y = act(acc + bias)
__device__ __forceinline__ void mfma_epilogue_fwd(
        const MfmaTile& t, const f32x16& a00, const f32x16& a01,
        const float* __restrict__ bias, float* __restrict__ y, int B, int out,
        int act_kind, int ksplit, float* __restrict__ parts) {
    mfma_cd_walk(a00, a01, [&](int r, int c, float acc) {
        int gm = t.m0 + r, gn = t.n0 + c;
        if (gm < B && gn < out) {
            if (ksplit > 1) {
                parts[((long)t.seg * B + gm) * out + gn] = acc;
            } else {
                float v = acc + bias[gn];
                if (act_kind == ACT_RELU) v = fmaxf(v, 0.f);
                else if (act_kind == ACT_TANH) v = tanhf(v);
                y[(long)gm * out + gn] = v;
            }
        }
    });
}

// dX: dx = acc * act'(hprev); hprev / dx are [B][span], hprev null => no mask
__device__ __forceinline__ void mfma_epilogue_dx(
        const MfmaTile& t, const f32x16& a00, const f32x16& a01,
        const float* __restrict__ hprev, float* __restrict__ dx, int B,
        int span, int prev_act) {
    mfma_cd_walk(a00, a01, [&](int r, int c, float acc) {
        int gm = t.m0 + r, gn = t.n0 + c;
        if (gm < B && gn < span) {
            long rel = (long)gm * span + gn;
            float m_ = hprev ? act_mask(prev_act, hprev[rel]) : 1.f;
            dx[rel] = acc * m_;
        }
    });
}

// dW: disjoint per-segment partials (k_dw_reduce sums) or the plain store;
// the waves with want_db (wave-uniform) also publish the column sums bias0 /
// bias1 of their B fragments as db, behind the ksplit weight partials.
__device__ __forceinline__ void mfma_epilogue_dw(
        const MfmaTile& t, const f32x16& a00, const f32x16& a01, float bias0,
        float bias1, bool want_db, float* __restrict__ dwt,
        float* __restrict__ db, int in_total, int out, int ksplit,
        float* __restrict__ parts) {
    mfma_cd_walk(a00, a01, [&](int r, int c, float acc) {
        int gi = t.m0 + r, go = t.n0 + c;
        if (gi < in_total && go < out) {
            if (ksplit > 1)
                parts[((long)t.seg * in_total + gi) * out + go] = acc;
            else
                dwt[(long)gi * out + go] = acc;
        }
    });
    if (want_db) {
        WavePos w;
        // combine the two k halves (lane l and l^32 share a column)
        bias0 += __shfl_xor(bias0, 32, 64);
        bias1 += __shfl_xor(bias1, 32, 64);
        if ((w.lane >> 5) == 0) {
            int go0 = t.n0 + w.wn0 + (w.lane & 31), go1 = go0 + 32;
            if (ksplit > 1) {
                long off = (long)ksplit * in_total * out + (long)t.seg * out;
                if (go0 < out) parts[off + go0] = bias0;
                if (go1 < out) parts[off + go1] = bias1;
            } else {
                if (go0 < out) db[go0] = bias0;
                if (go1 < out) db[go1] = bias1;
            }
        }
    }
}

}  // namespace d4pg
