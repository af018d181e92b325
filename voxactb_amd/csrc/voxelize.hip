// Deterministic multi-view point-cloud -> voxel-grid builder for gfx950 (MI355X).
//
// Replaces VoxelGrid.coords_to_bounding_voxel_grid (reference peract/voxel/voxel_grid.py:148-198,
// scatter-mean :106-146) and the per-camera flatten of QFunction.forward
// (peract/agents/peract_bc/qattention_peract_bc_agent.py:85-93).
//
// The reference zero-fills two dense B*(V+2)^3*7 accumulators, scatter-adds into both, divides,
// crops and concatenates: ~2.9 GB of traffic at B=16, V=100.  Here the dense grid is written exactly
// once and everything irregular happens on compact, L2-resident structures:
//
//   fill    pure 16-byte store stream: every cell written as "empty" (zeros | idx/V | 0)
//   count   1 thread / point: cell id, rank = atomicAdd(table[cell], 1); first toucher registers
//           the cell in a compact occupied-cell list               (int32 table, B*V^3*4 bytes)
//   alloc   1 thread / occupied cell: bump-allocate a segment of `count` ids, table[cell] = base
//   place   1 thread / point: seg[base + rank] = point id
//   reduce  1 thread / occupied cell (count <= 16): sort ids in registers (bitonic network), sum the
//           points IN ASCENDING POINT ID -- the order scatter_add_ uses on CPU -- divide, store the
//           cell's 10 floats, reset table[cell] = 0
//   reduce_long  1 wave / cell with count > 16: ids -> LDS bitmap (sorting by construction), expand,
//           batched gathers, sequential fp32 adds in id order
//
// Integer atomics only => run-to-run deterministic, and bit-identical to the CPU reference in all
// channels.  fp32 semantics follow the reference op for op (true division, the two +1e-12 terms).
//
// Since round 2 the chain above is the FALLBACK (F > 4 features, V > 200, N >= 2^20): the default point chain is the
// tile-routed one in voxelize_tiles.hip (no dense table, no sort, stable ballot ranks), which runs on a side stream next
// to the `fill` store stream of this file and patches the occupied cells in afterwards.
#include "voxelize.h"
#include <limits.h>
#include <stdlib.h>

namespace {

using VoxSrc = vox::Src;
using VoxGeom = vox::Geom;
constexpr int VOX_MAX_SRC = vox::MAX_SRC;
constexpr int VOX_MAX_F = vox::MAX_F;
constexpr int VOX_SHORT = 16;     // cells with <= this many points are reduced by one thread
constexpr int VOX_CHUNK = 2048;   // ids expanded per bitmap sweep in the long path (64 words x 32 bits)

struct VoxWs {
    int *table, *ctr, *occ_n, *cellid, *rank, *occ_cell, *occ_cnt, *occ_base, *seg, *longl;
    float* pdata;        // [B*N][8]: xyz, up to 4 features, point id (int bits) of every placed point, segment order
};
constexpr int VOX_PB = 1024;      // points (and occupied-cell slots) per block in count / alloc / reduce

__host__ __device__ inline size_t vox_ws_ints(long long B, long long N, long long V) {
    return (size_t)(B * V * V * V + 16 + ((B * N + VOX_PB - 1) / VOX_PB + 16) + 7 * B * N + 4 + 8 * B * N);
}

__host__ inline VoxWs vox_ws_carve(void* ws, long long B, long long N, long long V) {
    VoxWs w;
    int* p = (int*)ws;
    w.table = p;     p += B * V * V * V;
    w.ctr = p;       p += 16;
    w.occ_n = p;     p += (B * N + VOX_PB - 1) / VOX_PB + 16;
    w.cellid = p;    p += B * N;
    w.rank = p;      p += B * N;
    w.occ_cell = p;  p += B * N;
    w.occ_cnt = p;   p += B * N;
    w.occ_base = p;  p += B * N;
    w.seg = p;       p += B * N;
    w.longl = p;     p += B * N;
    w.pdata = (float*)(((uintptr_t)p + 15) & ~(uintptr_t)15);
    return w;
}

__device__ __forceinline__ int vox_axis_index(float p, float mn, float mx, int V) { return vox::axis_index(p, mn, mx, V); }
__device__ __forceinline__ const float* vox_point_ptr(const float* const* src, int n, int pps, int b, long long bs, long long ps) {
    return vox::point_ptr(src, n, pps, b, bs, ps);
}

// Same-address global atomics serialise at ~12 ns each on this chip (MI355X_MICROARCH "fanin"), so the
// occupied-cell list is kept per block: block k owns slots [k*VOX_PB, k*VOX_PB + occ_n[k]).
__global__ void __launch_bounds__(VOX_PB) vox_count_kernel(VoxSrc src, VoxGeom g, const float* __restrict__ bounds,
                                                           VoxWs w) {
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const long long t = (long long)blockIdx.x * VOX_PB + threadIdx.x;
    const bool live = t < (long long)g.B * g.N;
    int cell = -1, r = 0, gc = 0;
    if (live) {
        const int b = (int)(t / g.N);
        const int n = (int)(t - (long long)b * g.N);
        float pc[3];
        vox::load_coords(src, g, b, n, pc);
        const float* bd = bounds + (g.bounds_rows > 1 ? b * 6 : 0);
        int idx[3];
        bool inside = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int iv = vox_axis_index(pc[a], bd[a], bd[3 + a], g.V);
            inside = inside && (iv >= 1) && (iv <= g.V);
            idx[a] = iv - 1;
        }
        if (inside) {
            cell = (idx[0] * g.V + idx[1]) * g.V + idx[2];
            gc = b * g.V * g.V * g.V + cell;
            r = atomicAdd(&w.table[gc], 1);
        }
        w.cellid[t] = cell;
        w.rank[t] = r;
    }
    if (cell >= 0 && r == 0) {
        const int li = atomicAdd(&s_n, 1);
        w.occ_cell[(long long)blockIdx.x * VOX_PB + li] = gc;
    }
    __syncthreads();
    if (threadIdx.x == 0) w.occ_n[blockIdx.x] = s_n;
}

// Segment allocation: block-wide exclusive scan of the counts, ONE global atomicAdd per block.
__global__ void __launch_bounds__(VOX_PB) vox_alloc_kernel(VoxWs w) {
    __shared__ int s_wave[VOX_PB / 64];
    __shared__ int s_base, s_nlong, s_lbase;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) s_nlong = 0;
    const long long slot = (long long)blockIdx.x * VOX_PB + tid;
    const bool live = tid < w.occ_n[blockIdx.x];
    int gc = 0, L = 0;
    if (live) {
        gc = w.occ_cell[slot];
        L = w.table[gc];
    }
    int incl = L;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) s_wave[wid] = incl;
    __syncthreads();
    if (wid == 0) {
        int v = lane < VOX_PB / 64 ? s_wave[lane] : 0;
        int inc2 = v;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const int u = __shfl_up(inc2, o, 64);
            if (lane >= o) inc2 += u;
        }
        if (lane < VOX_PB / 64) s_wave[lane] = inc2 - v;
        if (lane == VOX_PB / 64 - 1) s_base = inc2 > 0 ? atomicAdd(&w.ctr[1], inc2) : 0;
    }
    __syncthreads();
    int lidx = -1;
    if (live) {
        const int base = s_base + s_wave[wid] + incl - L;
        w.table[gc] = base;
        w.occ_cnt[slot] = L;
        w.occ_base[slot] = base;
        if (L > VOX_SHORT) lidx = atomicAdd(&s_nlong, 1);
    }
    __syncthreads();
    if (tid == 0 && s_nlong > 0) s_lbase = atomicAdd(&w.ctr[2], s_nlong);
    __syncthreads();
    if (lidx >= 0) w.longl[s_lbase + lidx] = (int)slot;
}

__global__ void __launch_bounds__(256) vox_place_kernel(VoxGeom g, VoxWs w) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)g.B * g.N) return;
    const int cell = w.cellid[t];
    if (cell < 0) return;
    const int b = (int)(t / g.N);
    const int n = (int)(t - (long long)b * g.N);
    const int base = w.table[b * g.V * g.V * g.V + cell];
    w.seg[base + w.rank[t]] = n;
}

#define VOX_CSWAP(x, y)            \
    {                              \
        const int lo_ = min(x, y); \
        const int hi_ = max(x, y); \
        x = lo_;                   \
        y = hi_;                   \
    }

__device__ __forceinline__ void vox_sort16(int (&a)[16]) {
    // bitonic network, fully unrolled so that a[] stays in registers
#pragma unroll
    for (int k = 2; k <= 16; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    if ((i & k) == 0) { VOX_CSWAP(a[i], a[l]); }
                    else { VOX_CSWAP(a[l], a[i]); }
                }
            }
        }
    }
}

template <int F>
__device__ __forceinline__ void vox_store_cell(float* __restrict__ out, int gc, int V, const float (&acc)[3 + F], int L) {
    constexpr int C = 3 + F + 4;
    const int V3 = V * V * V;
    const int cell = gc % V3;
    const int x = cell / (V * V);
    const int y = (cell / V) % V;
    const int z = cell % V;
    float* o = out + (size_t)gc * C;
    const float Lf = (float)L;                       // clamp_(1) is a no-op for occupied cells (:121)
#pragma unroll
    for (int c = 0; c < 3 + F; ++c) o[c] = __fdiv_rn(acc[c], Lf);
    const float Vf = (float)V;                       // self._voxel_d (:197)
    o[3 + F + 0] = __fdiv_rn((float)x, Vf);
    o[3 + F + 1] = __fdiv_rn((float)y, Vf);
    o[3 + F + 2] = __fdiv_rn((float)z, Vf);
    o[3 + F + 3] = 1.0f;                             // (count/count > 0).float()  (:192)
}

template <int F>
__global__ void __launch_bounds__(256) vox_reduce_short_kernel(VoxSrc src, VoxGeom g, VoxWs w, float* __restrict__ out) {
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if ((slot % VOX_PB) >= w.occ_n[slot / VOX_PB]) return;
    const int L = w.occ_cnt[slot];
    if (L > VOX_SHORT) return;
    const int gc = w.occ_cell[slot];
    const int base = w.occ_base[slot];
    const int b = gc / (g.V * g.V * g.V);
    int a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = (i < L) ? w.seg[base + i] : INT_MAX;
    if (L == 2) {
        VOX_CSWAP(a[0], a[1]);
    } else if (L > 2) {
        vox_sort16(a);
    }
    float acc[3 + F];
#pragma unroll
    for (int c = 0; c < 3 + F; ++c) acc[c] = 0.0f;     // zeros_like(self._flat_output) (:145)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (i < L) {
            float pc[3];
            vox::load_coords(src, g, b, a[i], pc);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = __fadd_rn(acc[c], pc[c]);
            if (F > 0) {
                const float* fp = vox_point_ptr(src.f, a[i], g.pps, b, g.fb, g.fp);
#pragma unroll
                for (int c = 0; c < F; ++c) acc[3 + c] = __fadd_rn(acc[3 + c], fp[c * g.fc]);
            }
        }
    }
    vox_store_cell<F>(out, gc, g.V, acc, L);
    w.table[gc] = 0;
}

// ---- data-carrying variant (F <= 4, N < 2^27): `place` also copies the point's coordinates / features / id into its
// 32-byte slot of the cell's segment (coalesced reads, fire-and-forget scatter stores), so that the reduction streams
// contiguous 32-byte records instead of gathering 3 + F scattered words per point.  Same ascending-id summation order.
template <int F>
__global__ void __launch_bounds__(256) vox_place_data_kernel(VoxSrc src, VoxGeom g, VoxWs w) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)g.B * g.N) return;
    const int cell = w.cellid[t];
    if (cell < 0) return;
    const int b = (int)(t / g.N);
    const int n = (int)(t - (long long)b * g.N);
    const int slot = w.table[b * g.V * g.V * g.V + cell] + w.rank[t];
    w.seg[slot] = n;
    float v[8];
    {
        float pc[3];
        vox::load_coords(src, g, b, n, pc);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = pc[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) v[3 + c] = 0.f;
    if (F > 0) {
        const float* fp = vox_point_ptr(src.f, n, g.pps, b, g.fb, g.fp);
#pragma unroll
        for (int c = 0; c < F; ++c) v[3 + c] = fp[c * g.fc];
    }
    v[7] = __int_as_float(n);
    float4* pd = reinterpret_cast<float4*>(w.pdata + (size_t)slot * 8);
    pd[0] = make_float4(v[0], v[1], v[2], v[3]);
    pd[1] = make_float4(v[4], v[5], v[6], v[7]);
}

template <int F>
__global__ void __launch_bounds__(256) vox_reduce_short_pd_kernel(VoxGeom g, VoxWs w, float* __restrict__ out) {
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if ((slot % VOX_PB) >= w.occ_n[slot / VOX_PB]) return;
    const int L = w.occ_cnt[slot];
    if (L > VOX_SHORT) return;
    const int gc = w.occ_cell[slot];
    const float4* pd = reinterpret_cast<const float4*>(w.pdata + (size_t)w.occ_base[slot] * 8);
    float acc[3 + F];
#pragma unroll
    for (int c = 0; c < 3 + F; ++c) acc[c] = 0.0f;     // zeros_like(self._flat_output) (:145)
    if (L == 1) {
        const float4 a0 = pd[0], a1 = pd[1];
        const float r[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int c = 0; c < 3 + F; ++c) acc[c] = __fadd_rn(acc[c], r[c]);
    } else {
        int a[16];                                     // (id << 4) | record index: sorting the keys sorts by id
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = (i < L) ? ((__float_as_int(pd[2 * i + 1].w) << 4) | i) : INT_MAX;
        if (L == 2) {
            VOX_CSWAP(a[0], a[1]);
        } else {
            vox_sort16(a);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < L) {
                const int k = a[i] & 15;
                const float4 a0 = pd[2 * k], a1 = pd[2 * k + 1];
                const float r[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
                for (int c = 0; c < 3 + F; ++c) acc[c] = __fadd_rn(acc[c], r[c]);
            }
        }
    }
    vox_store_cell<F>(out, gc, g.V, acc, L);
    w.table[gc] = 0;
}

template <int F>
__global__ void __launch_bounds__(64) vox_reduce_long_kernel(VoxSrc src, VoxGeom g, VoxWs w, float* __restrict__ out,
                                                            int n_words) {
    constexpr int NC = 3 + F;
    constexpr int C = NC + 4;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    unsigned* bm = (unsigned*)smem;
    int* chunk = smem + ((n_words + 63) & ~63);
    float* stage = (float*)(chunk + VOX_CHUNK);
    const int lane = threadIdx.x;
    const int n_long = w.ctr[2];
    const int V3 = g.V * g.V * g.V;
    for (int li = blockIdx.x; li < n_long; li += gridDim.x) {
        const int slot = w.longl[li];
        const int gc = w.occ_cell[slot];
        const int L = w.occ_cnt[slot];
        const int base = w.occ_base[slot];
        const int b = gc / V3;
        for (int i = lane; i < n_words; i += 64) bm[i] = 0u;
        __syncthreads();
        for (int i = lane; i < L; i += 64) {
            const int id = w.seg[base + i];
            atomicOr(&bm[id >> 5], 1u << (id & 31));
        }
        __syncthreads();
        float acc = 0.0f;                     // lane c < NC accumulates channel c
        for (int w0 = 0; w0 < n_words; w0 += 64) {
            const int wi = w0 + lane;
            unsigned word = (wi < n_words) ? bm[wi] : 0u;
            const int cnt = __popc(word);
            int incl = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            const int total = __shfl(incl, 63, 64);
            if (total == 0) continue;          // wave-uniform
            int pos = incl - cnt;
            while (word) {
                const int bit = __ffs(word) - 1;
                chunk[pos++] = (wi << 5) + bit;
                word &= word - 1;
            }
            __syncthreads();
            for (int k0 = 0; k0 < total; k0 += 64) {
                const int m = min(64, total - k0);
                if (lane < m) {
                    const int n = chunk[k0 + lane];
                    float pc[3];
                    vox::load_coords(src, g, b, n, pc);
#pragma unroll
                    for (int c = 0; c < 3; ++c) stage[lane * NC + c] = pc[c];
                    if (F > 0) {
                        const float* fp = vox_point_ptr(src.f, n, g.pps, b, g.fb, g.fp);
#pragma unroll
                        for (int c = 0; c < F; ++c) stage[lane * NC + 3 + c] = fp[c * g.fc];
                    }
                }
                __syncthreads();
                if (lane < NC) {
                    for (int j = 0; j < m; ++j) acc = __fadd_rn(acc, stage[j * NC + lane]);
                }
                __syncthreads();
            }
        }
        const int cell = gc % V3;
        float* o = out + (size_t)gc * C;
        const float Vf = (float)g.V;
        if (lane < NC) o[lane] = __fdiv_rn(acc, (float)L);
        else if (lane == NC) o[lane] = __fdiv_rn((float)(cell / (g.V * g.V)), Vf);
        else if (lane == NC + 1) o[lane] = __fdiv_rn((float)((cell / g.V) % g.V), Vf);
        else if (lane == NC + 2) o[lane] = __fdiv_rn((float)(cell % g.V), Vf);
        else if (lane == NC + 3) o[lane] = 1.0f;
        if (lane == 0) w.table[gc] = 0;
        __syncthreads();
    }
}

// Every cell as "empty": channels [0, NC) = 0, idx/V, occupancy 0 (voxel_grid.py:192-198 for count == 0).
// One z-row (V*C floats) per block iteration, 16-byte stores; the (z, channel) of a thread's four
// floats do not depend on the row, so they are decoded once.
__global__ void __launch_bounds__(256) vox_fill_kernel(float* __restrict__ out, int rows, int V, int C) {
    constexpr int RB = 8;                          // consecutive rows per block step: 8 * V*C*4 B is a
    const int NC = C - 4;                          // multiple of 128 B for even V*C/4 ... keeps lines whole
    const int q4 = (V * C) >> 2;                 // float4 per row
    const float Vf = (float)V;
    const int groups = (rows + RB - 1) / RB;
    for (int j = threadIdx.x; j < q4; j += 256) {
        int sel[4];
        float zv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int f = 4 * j + e;
            const int z = f / C;
            const int ch = f - z * C;
            sel[e] = ch - NC;                      // 0 -> x/V, 1 -> y/V, 2 -> z/V, else 0
            zv[e] = __fdiv_rn((float)z, Vf);
        }
        for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
#pragma unroll
            for (int rr = 0; rr < RB; ++rr) {
                const int row = grp * RB + rr;
                if (row < rows) {
                    const int xy = row % (V * V);
                    const float xv = __fdiv_rn((float)(xy / V), Vf);
                    const float yv = __fdiv_rn((float)(xy % V), Vf);
                    float4 v;
                    v.x = sel[0] == 0 ? xv : sel[0] == 1 ? yv : sel[0] == 2 ? zv[0] : 0.0f;
                    v.y = sel[1] == 0 ? xv : sel[1] == 1 ? yv : sel[1] == 2 ? zv[1] : 0.0f;
                    v.z = sel[2] == 0 ? xv : sel[2] == 1 ? yv : sel[2] == 2 ? zv[2] : 0.0f;
                    v.w = sel[3] == 0 ? xv : sel[3] == 1 ? yv : sel[3] == 2 ? zv[3] : 0.0f;
                    reinterpret_cast<float4*>(out + (size_t)row * V * C)[j] = v;   // plain: nt measured slower
                }
            }
        }
    }
}

// C = 10 (xyz, rgb, index, occupancy), V even: the same values as one FLAT, 16-byte aligned store stream per sample
// (every wave instruction writes one aligned 1 KB run; the row-wise kernel above starts a row every 4000 bytes and ends
// each on a partial wave: 5.0 vs 5.9-6.4 TB/s in tools/ubench/storebw.hip).  The pattern repeats every 20 floats = two
// cells = five float4: j = 0, 3 are all zero, j = 1 carries (x, y)/V of the first cell, j = 2 its z/V, j = 4 the second
// cell's (x, y, z)/V.  k/V comes from an LDS table (IEEE division once per block), the cell coordinates from
// multiply-high divisions (cell * V < 2^32, checked by the host).
__global__ void __launch_bounds__(256) vox_fill_flat10_kernel(float* __restrict__ out, unsigned n4, int V, unsigned magicV) {
    extern __shared__ float vtab[];
    for (int k = threadIdx.x; k < V; k += 256) vtab[k] = __fdiv_rn((float)k, (float)V);
    __syncthreads();
    float4* __restrict__ o = reinterpret_cast<float4*>(out + (size_t)blockIdx.y * n4 * 4);
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const unsigned grp = i / 5u, j = i - 5u * grp;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j == 1u || j == 2u || j == 4u) {
            const unsigned cell = 2u * grp + (j == 4u ? 1u : 0u);
            const unsigned xy = __umulhi(cell, magicV), z = cell - xy * (unsigned)V;
            const unsigned x = __umulhi(xy, magicV), y = xy - x * (unsigned)V;
            if (j == 1u) { v.z = vtab[x]; v.w = vtab[y]; }
            else if (j == 2u) { v.x = vtab[z]; }
            else { v.x = vtab[x]; v.y = vtab[y]; v.z = vtab[z]; }
        }
        o[i] = v;
    }
}

// generic fallback when V*C is not a multiple of 4 (odd V): one float per thread iteration
__global__ void __launch_bounds__(256) vox_fill_scalar_kernel(float* __restrict__ out, long long total, int V, int C) {
    const int NC = C - 4;
    const float Vf = (float)V;
    for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < total; f += (long long)gridDim.x * 256) {
        const long long cellg = f / C;
        const int ch = (int)(f - cellg * C);
        const int cell = (int)(cellg % ((long long)V * V * V));
        float v = 0.0f;
        if (ch == NC) v = __fdiv_rn((float)(cell / (V * V)), Vf);
        else if (ch == NC + 1) v = __fdiv_rn((float)((cell / V) % V), Vf);
        else if (ch == NC + 2) v = __fdiv_rn((float)(cell % V), Vf);
        out[f] = v;
    }
}

template <int F>
int vox_launch_reduce(const VoxSrc& src, const VoxGeom& g, const VoxWs& w, float* out, hipStream_t st, hipStream_t st_long,
                      bool use_pd) {
    // short cells on `st`, the few long cells (one wave each, latency-bound) on `st_long`: they write disjoint cells
    const long long BN = (long long)g.B * g.N;
    if (use_pd && F <= 4) hipLaunchKernelGGL(vox_reduce_short_pd_kernel<(F <= 4 ? F : 0)>, dim3(vxb_cdiv(BN, 256)), dim3(256), 0, st, g, w, out);
    else hipLaunchKernelGGL(vox_reduce_short_kernel<F>, dim3(vxb_cdiv(BN, 256)), dim3(256), 0, st, src, g, w, out);
    const int n_words = (g.N + 31) / 32;
    const size_t lds = (size_t)(((n_words + 63) & ~63) + VOX_CHUNK) * 4 + (size_t)64 * (3 + F) * 4;
    if (lds > 160 * 1024) return VXB_ESIZE;
    if (lds > 64 * 1024) {
        if (hipFuncSetAttribute((const void*)vox_reduce_long_kernel<F>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds) != hipSuccess)
            return VXB_ELAUNCH;
    }
    const int grid = (int)(BN / (VOX_SHORT + 1) < 1 ? 1 : (BN / (VOX_SHORT + 1) > 2048 ? 2048 : BN / (VOX_SHORT + 1)));
    hipLaunchKernelGGL(vox_reduce_long_kernel<F>, dim3(grid), dim3(64), lds, st_long, src, g, w, out, n_words);
    return VXB_OK;
}

}  // namespace

extern "C" int vxb_abi_version(void) { return 6; }      // 6: the 15 slope-only backward / pointwise entries of ABI 4 removed (their *_act_f32 forms stay); 5: activation code 2 (tanh) + the *_act_f32 backward entries; 4 (round 6): + vxb_gemm_wide_geglu_bwd_f16x2_f32, vxb_gemm_wide_bf16x3_f16out_f32; 3: vxb_patch_dgrad_input_wgrad_f32 gained dWp / ws_wp in round 5 (advisor), + the *_mask attention entries

namespace {
struct VoxStreams {
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_placed = nullptr, ev_long = nullptr;
};
// one set per device (a process normally drives one GPU; the table keeps a multi-device process correct)
int vox_streams(VoxStreams** out) {
    static VoxStreams tab[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return VXB_ELAUNCH;
    VoxStreams& s = tab[dev];
    if (!s.side) {
        // highest priority: the point chain's few small workgroups must not queue behind the 156 k workgroups of the fill
        int prio_lo = 0, prio_hi = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) prio_hi = 0;
        if (hipStreamCreateWithPriority(&s.side, hipStreamNonBlocking, prio_hi) != hipSuccess) return VXB_ELAUNCH;
        if (hipEventCreateWithFlags(&s.ev_fork, hipEventDisableTiming) != hipSuccess) return VXB_ELAUNCH;
        if (hipEventCreateWithFlags(&s.ev_join, hipEventDisableTiming) != hipSuccess) return VXB_ELAUNCH;
        if (hipEventCreateWithFlags(&s.ev_placed, hipEventDisableTiming) != hipSuccess) return VXB_ELAUNCH;
        if (hipEventCreateWithFlags(&s.ev_long, hipEventDisableTiming) != hipSuccess) return VXB_ELAUNCH;
    }
    *out = &s;
    return VXB_OK;
}

int g_vox_chain = -1;        // -1: not decided yet (environment), 0: automatic, 1: always the table-based chain, 3 / 5: see header
bool vox_force_table_chain() {
    if (g_vox_chain < 0) {
        const char* e = getenv("VXB_VOXELIZE_TABLE");       // debugging / A-B switch, same values as vxb_voxelize_select_chain
        g_vox_chain = (e && (e[0] == '1' || e[0] == '3' || e[0] == '5')) ? e[0] - '0' : 0;
    }
    return g_vox_chain == 1;
}

}  // namespace
void vox_launch_fill(float* out, int B, int V, int C, hipStream_t fs) {
    const long long V3 = (long long)V * V * V;
    if (C == 10 && (V & 1) == 0 && V >= 2 && V <= 1024 && (((uintptr_t)out) & 15) == 0 && V3 * V < (1ll << 32)) {
        const unsigned n4 = (unsigned)(V3 * 10 / 4);                    // float4 per sample
        const unsigned magicV = (unsigned)((1ull << 32) / (unsigned)V) + 1u;
        const unsigned gx = (n4 + 255) / 256;       // one float4 per thread: many short blocks sustain 6.4 TB/s, few long ones 4.7
        hipLaunchKernelGGL(vox_fill_flat10_kernel, dim3(gx, B), dim3(256), V * sizeof(float), fs, out, n4, V, magicV);
    } else if (((V * C) & 3) == 0 && (((uintptr_t)out) & 15) == 0) {
        const int rows = B * V * V;
        const int groups = (rows + 7) / 8;
        hipLaunchKernelGGL(vox_fill_kernel, dim3(groups), dim3(256), 0, fs, out, rows, V, C);
    } else {
        hipLaunchKernelGGL(vox_fill_scalar_kernel, dim3(2048), dim3(256), 0, fs, out, (long long)B * V3 * C, V, C);
    }
}

extern "C" int vxb_voxelize_select_chain(int which) {
    if (which != 0 && which != 1 && which != 3 && which != 5 && which != 7) return VXB_EARG;
    g_vox_chain = which;
    return VXB_OK;
}

extern "C" size_t vxb_voxelize_workspace_bytes(int B, int n_points, int V) {
    if (B <= 0 || n_points <= 0 || V <= 0) return 0;
    const size_t table = vox_ws_ints(B, n_points, V) * sizeof(int);
    const size_t tiles = vox_tiles_ws_bytes(B, n_points, V);
    return table > tiles ? table : tiles;
}

static int vox_run(const float* const* coord_src, const float* const* feat_src, int n_src,
                   int B, int pts_per_src, int F,
                   int64_t coord_bstride, int64_t coord_cstride, int64_t coord_pstride,
                   int64_t feat_bstride, int64_t feat_cstride, int64_t feat_pstride,
                   const float* bounds, int bounds_rows, int V, const float* xform, const double* proj, int img_w, int depth_norm,
                   float* out, int out_state, void* workspace, size_t workspace_bytes, vxb_stream_t stream) {
    if (!coord_src || !bounds || !out || !workspace) return VXB_EARG;
    if (n_src < 1 || n_src > VOX_MAX_SRC || B < 1 || pts_per_src < 1 || V < 1) return VXB_EARG;
    if (F < 0 || F > VOX_MAX_F || (F > 0 && !feat_src)) return VXB_EARG;
    if (bounds_rows != 1 && bounds_rows != B) return VXB_EARG;
    if (out_state < 0 || out_state > 2) return VXB_EARG;
    const long long N = (long long)n_src * pts_per_src;
    const long long V3 = (long long)V * V * V;
    if ((long long)B * V3 >= INT_MAX || (long long)B * N >= INT_MAX) return VXB_ESIZE;
    if (workspace_bytes < vxb_voxelize_workspace_bytes(B, (int)N, V)) return VXB_EWS;
    hipStream_t st = (hipStream_t)stream;
    VoxSrc src;
    for (int s = 0; s < VOX_MAX_SRC; ++s) {
        src.c[s] = s < n_src ? coord_src[s] : nullptr;
        src.f[s] = (s < n_src && F > 0) ? feat_src[s] : nullptr;
        if (s < n_src && (!src.c[s] || (F > 0 && !src.f[s]))) return VXB_EARG;
    }
    VoxGeom g;
    g.B = B; g.n_src = n_src; g.pps = pts_per_src; g.N = (int)N; g.F = F; g.V = V; g.bounds_rows = bounds_rows;
    g.cb = coord_bstride; g.cc = coord_cstride; g.cp = coord_pstride;
    g.fb = feat_bstride; g.fc = feat_cstride; g.fp = feat_pstride;
    g.xf = xform;
    g.proj = proj; g.img_w = img_w; g.depth_norm = depth_norm;
    const int C = 3 + F + 4;
    const long long BN = (long long)B * N;
    VoxStreams* vs = nullptr;
    if (vox_streams(&vs) != VXB_OK) return VXB_ELAUNCH;
    hipStream_t fs = vs->side;

    if (vox_tiles_supported(B, N, V, F) && !vox_force_table_chain()) {
        // the point chain (route -> light / heavy tiles) runs on the side stream next to the dense "empty grid" store
        // stream, joins, and the occupied cells are patched in
        // out_state 1 / 2: `out` and `workspace` are exactly as the previous successful call with the same geometry left them
        // -> incremental update (no fill).  Orders 0 / 3 overlap the fill with the point chain; measured on MI355X that
        // overlap buys nothing (the store stream stretches the latency-bound chain by what it hides), so a stateless call
        // runs the fill after the chain.
        // g_vox_chain 0 (default): round 5's merged tile launch (orders 6 / 7; they fall back to 2 / 4 where they do not apply);
        // 3: round 4's chain (fill, route, classify, heavy, light as separate launches: orders 2 / 4), 5: the fill on a side stream
        // 7 (A/B): round 5's incremental chain (unpatch as its own launch); since round 6 the default resets the old cells inside the route launch (order 9)
        const int order = out_state != 0 ? (g_vox_chain == 0 ? 9 : g_vox_chain == 7 ? 7 : 4) : (g_vox_chain == 5 ? 0 : (g_vox_chain == 3 ? 2 : 6));
        // out_state 0 / 2 -> this call writes cell list 0, out_state 1 -> list 1 (and resets the cells of the other one)
        return vox_tiles_launch(src, g, bounds, out, workspace, st, fs, vs->ev_fork, vs->ev_placed, vs->ev_join, order,
                                out_state == 1 ? 0 : (out_state == 2 ? 1 : -1), out_state == 1 ? 1 : 0);
    }

    // ---- table-based fallback chain
    VoxWs w = vox_ws_carve(workspace, B, N, V);
    // the count table must be zero on entry (the chain leaves it zero, but the workspace is shared with the tile chain)
    if (hipMemsetAsync(w.table, 0, (size_t)B * V3 * sizeof(int), st) != hipSuccess) return VXB_ELAUNCH;
    if (hipMemsetAsync(w.ctr, 0, 16 * sizeof(int), st) != hipSuccess) return VXB_ELAUNCH;
    if (hipEventRecord(vs->ev_fork, st) != hipSuccess || hipStreamWaitEvent(fs, vs->ev_fork, 0) != hipSuccess) return VXB_ELAUNCH;
    vox_launch_fill(out, B, V, C, fs);
    hipLaunchKernelGGL(vox_count_kernel, dim3(vxb_cdiv(BN, VOX_PB)), dim3(VOX_PB), 0, st, src, g, bounds, w);
    hipLaunchKernelGGL(vox_alloc_kernel, dim3(vxb_cdiv(BN, VOX_PB)), dim3(VOX_PB), 0, st, w);
    const bool use_pd = F <= 4 && N < (1ll << 27);     // records of 8 floats; (id << 4 | index) sort keys
    if (use_pd) {
        switch (F) {
            case 0: hipLaunchKernelGGL(vox_place_data_kernel<0>, dim3(vxb_cdiv(BN, 256)), dim3(256), 0, st, src, g, w); break;
            case 1: hipLaunchKernelGGL(vox_place_data_kernel<1>, dim3(vxb_cdiv(BN, 256)), dim3(256), 0, st, src, g, w); break;
            case 2: hipLaunchKernelGGL(vox_place_data_kernel<2>, dim3(vxb_cdiv(BN, 256)), dim3(256), 0, st, src, g, w); break;
            case 3: hipLaunchKernelGGL(vox_place_data_kernel<3>, dim3(vxb_cdiv(BN, 256)), dim3(256), 0, st, src, g, w); break;
            default: hipLaunchKernelGGL(vox_place_data_kernel<4>, dim3(vxb_cdiv(BN, 256)), dim3(256), 0, st, src, g, w); break;
        }
    } else {
        hipLaunchKernelGGL(vox_place_kernel, dim3(vxb_cdiv(BN, 256)), dim3(256), 0, st, g, w);
    }
    // the side stream (fill done) also runs the long-cell reduction once the segments are placed
    if (hipEventRecord(vs->ev_placed, st) != hipSuccess || hipEventRecord(vs->ev_join, fs) != hipSuccess) return VXB_ELAUNCH;
    if (hipStreamWaitEvent(st, vs->ev_join, 0) != hipSuccess || hipStreamWaitEvent(fs, vs->ev_placed, 0) != hipSuccess) return VXB_ELAUNCH;
    int rc = VXB_OK;
    switch (F) {
        case 0: rc = vox_launch_reduce<0>(src, g, w, out, st, fs, use_pd); break;
        case 1: rc = vox_launch_reduce<1>(src, g, w, out, st, fs, use_pd); break;
        case 2: rc = vox_launch_reduce<2>(src, g, w, out, st, fs, use_pd); break;
        case 3: rc = vox_launch_reduce<3>(src, g, w, out, st, fs, use_pd); break;
        case 4: rc = vox_launch_reduce<4>(src, g, w, out, st, fs, use_pd); break;
        case 5: rc = vox_launch_reduce<5>(src, g, w, out, st, fs, use_pd); break;
        case 6: rc = vox_launch_reduce<6>(src, g, w, out, st, fs, use_pd); break;
        case 7: rc = vox_launch_reduce<7>(src, g, w, out, st, fs, use_pd); break;
        case 8: rc = vox_launch_reduce<8>(src, g, w, out, st, fs, use_pd); break;
        default: return VXB_EARG;
    }
    if (rc != VXB_OK) return rc;
    if (hipEventRecord(vs->ev_long, fs) != hipSuccess || hipStreamWaitEvent(st, vs->ev_long, 0) != hipSuccess) return VXB_ELAUNCH;
    VXB_CHECK_LAUNCH();
    return VXB_OK;
}

extern "C" int vxb_voxelize_f32(const float* const* coord_src, const float* const* feat_src, int n_src,
                                int B, int pts_per_src, int F,
                                int64_t coord_bstride, int64_t coord_cstride, int64_t coord_pstride,
                                int64_t feat_bstride, int64_t feat_cstride, int64_t feat_pstride,
                                const float* bounds, int bounds_rows, int V, const float* xform,
                                float* out, int out_state, void* workspace, size_t workspace_bytes, vxb_stream_t stream) {
    return vox_run(coord_src, feat_src, n_src, B, pts_per_src, F, coord_bstride, coord_cstride, coord_pstride, feat_bstride,
                   feat_cstride, feat_pstride, bounds, bounds_rows, V, xform, nullptr, 0, 0, out, out_state, workspace,
                   workspace_bytes, stream);
}

extern "C" int vxb_voxelize_depth_f32(const float* const* depth_src, const float* const* feat_src, int n_src, int B, int H, int W,
                                      int F, int64_t feat_bstride, int64_t feat_cstride, int64_t feat_pstride, const double* proj,
                                      int depth_normalised, const float* bounds, int bounds_rows, int V, const float* xform,
                                      float* out, int out_state, void* workspace, size_t workspace_bytes, vxb_stream_t stream) {
    if (!proj || H < 1 || W < 1) return VXB_EARG;
    return vox_run(depth_src, feat_src, n_src, B, H * W, F, (int64_t)H * W, 0, 1, feat_bstride, feat_cstride, feat_pstride, bounds,
                   bounds_rows, V, xform, proj, W, depth_normalised ? 1 : 0, out, out_state, workspace, workspace_bytes, stream);
}
