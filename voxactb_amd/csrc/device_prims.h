// Device primitives shared by the MFMA kernels (attention, GEMM, conv): one definition of each, all force-inlined.  Internal, like
// common.h.  Only helpers whose bodies were the same in every kernel live here; a helper with semantics of its own stays in its file.
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

// ---- attention dropout mask
// The forward kernels draw the mask and every backward kernel rebuilds it from the same hash, so this is the ONE definition both sides
// must agree on.  Key pair (2c, 2c+1) of query row `row` is hashed once: vxb_drop_hash((row * 0x9E3779B1 + seed) ^ (c * 0x85EBCA77 +
// 0xC2B2AE3D)); the low 16 bits decide key 2c, the high 16 bits key 2c+1, and a key is KEPT when its field is >= thr = (unsigned)(p * 65536)
// (the flash2_* kernels hoist the row term, `rowh`, and the column term, `colb`, out of their loops; the value hashed is the same).
// One multiply round: the inputs are already products with odd constants; keep-rate, row / column sums and lag correlations of the
// 16-bit halves are indistinguishable from the two-round finaliser (checked offline on 4096 x 2048 masks), and every hash costs a
// quarter-rate multiply less in the softmax loops.
__device__ __forceinline__ unsigned vxb_drop_hash(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15;
    return x;
}
__device__ __forceinline__ unsigned vxb_drop_keep_pair(unsigned seed, unsigned row, unsigned colpair) {
    return vxb_drop_hash((row * 0x9E3779B1U + seed) ^ (colpair * 0x85EBCA77U + 0xC2B2AE3DU));
}

// ---- 16-bit operand fragments
enum { M_BF16 = 0, M_F16 = 1 };       // element type of a 16-bit operand plane

__device__ __forceinline__ bf16x8 vxb_join(unsigned long long a, unsigned long long b) {
    union { unsigned long long u[2]; bf16x8 v; } t;
    t.u[0] = a; t.u[1] = b;
    return t.v;
}
__device__ __forceinline__ bf16x8 vxb_from4(const unsigned* p) {
    union { unsigned u[4]; bf16x8 v; } t;
    t.u[0] = p[0]; t.u[1] = p[1]; t.u[2] = p[2]; t.u[3] = p[3];
    return t.v;
}
__device__ __forceinline__ bf16x8 vxb_from4(unsigned a, unsigned b, unsigned c, unsigned d) {
    union { unsigned u[4]; bf16x8 v; } t;
    t.u[0] = a; t.u[1] = b; t.u[2] = c; t.u[3] = d;
    return t.v;
}
// hi/lo split of a value pair: ph = bf16 pair, pl = bf16 pair of the (exact) residuals
__device__ __forceinline__ void vxb_split2(float a, float b, unsigned& ph, unsigned& pl) {
    ph = vxb_pack_bf16(a, b);
    pl = vxb_pack_bf16(a - __uint_as_float(ph << 16), b - __uint_as_float(ph & 0xffff0000u));
}
// 8 consecutive fp32 (two float4) -> one bf16x8 fragment (+ residual fragment when X3), pre-scaled by s
template <int X3>
__device__ __forceinline__ void vxb_frag8(const float* p, float s, bf16x8& fh, bf16x8& fl) {
    union { unsigned u[4]; bf16x8 v; } h, l;
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 c = *reinterpret_cast<const float4*>(p + 4);
    if (X3) {
        vxb_split2(a.x * s, a.y * s, h.u[0], l.u[0]); vxb_split2(a.z * s, a.w * s, h.u[1], l.u[1]);
        vxb_split2(c.x * s, c.y * s, h.u[2], l.u[2]); vxb_split2(c.z * s, c.w * s, h.u[3], l.u[3]);
        fl = l.v;
    } else {
        h.u[0] = vxb_pack_bf16(a.x * s, a.y * s); h.u[1] = vxb_pack_bf16(a.z * s, a.w * s);
        h.u[2] = vxb_pack_bf16(c.x * s, c.y * s); h.u[3] = vxb_pack_bf16(c.z * s, c.w * s);
        fl = h.v;
    }
    fh = h.v;
}
// two fp32 -> one 16-bit pair of element type MODE, and the values a pack kept back as fp32
template <int MODE>
__device__ __forceinline__ unsigned vxb_pack(float a, float b) {
    return MODE == M_BF16 ? vxb_pack_bf16(a, b) : vxb_pack_f16(a, b);
}
template <int MODE>
__device__ __forceinline__ void vxb_unpack(unsigned p, float& a, float& b) {
    if (MODE == M_BF16) { a = __uint_as_float(p << 16); b = __uint_as_float(p & 0xffff0000u); }
    else {
        union { unsigned u; vxb_f16x2 h; } t; t.u = p;
        a = (float)t.h[0]; b = (float)t.h[1];
    }
}
// transposed 8-byte LDS read through the compiler builtin: a lane base + compile-time offset folds into the instruction's immediate
// (no address arithmetic per read) and the compiler places the waits
__device__ __forceinline__ unsigned long long vxb_tr16(const u16* p) {
    union { s16x4 v; unsigned long long u; } t;
    t.v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)p);
    return t.u;
}
// two transposed 8-byte LDS reads -> one 16-bit fragment
__device__ __forceinline__ bf16x8 vxb_frag(const u16* p0, const u16* p1) {
    union { s16x4 s[2]; bf16x8 v; } t;
    t.s[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p0));
    t.s[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p1));
    return t.v;
}
// 16-byte chunk XOR key of row `row` of a 64 x 64 16-bit tile: conflict-free for ds_read_b128 AND for the transposed reads
__device__ __forceinline__ int vxb_swz(int row) {
    const int x = (row >> 1) & 7;
    return ((x & 1) << 2) | (x >> 1);
}

// ---- 32x32 MFMA products
// acc += A B, one product of 16-bit operands of element type MODE
template <int MODE>
__device__ __forceinline__ f32x16 vxb_mma(const bf16x8 a, const bf16x8 b, f32x16 c) {
    if (MODE == M_BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// acc += A B with A = ah + al, B = bh + bl (X3: hi*hi + hi*lo + lo*hi) or A = ah, B = bh
template <int X3>
__device__ __forceinline__ f32x16 vxb_mma_x3(const bf16x8 ah, const bf16x8 al, const bf16x8 bh, const bf16x8 bl, f32x16 c) {
    if (X3) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
}

// ---- direct global -> LDS loads
// Through the compiler builtin: 16 bytes per lane, src -> LDS[lds_wave_base + 16 lane].  The compiler knows the load and places its waits.
__device__ __forceinline__ void vxb_load_lds16(const u16* src, u16* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
// As INLINE ASM: lane l's 16 (dwordx4) or 4 (dword) bytes at base + byte_off -> LDS[lds_wave_base + 16 l (4 l)]; base and lds_wave_base
// are wave-uniform (SGPRs), byte_off is the lane's offset (VGPR).  The contract:
//  * Why asm: the compiler's waitcnt pass orders every later LDS read behind a direct-to-LDS load it knows about (an s_waitcnt vmcnt(0)
//    in front of the first LDS read that may alias the destination), which drains the loads a pipelined kernel keeps in flight on
//    purpose.  Issued as asm the load is invisible to that pass.
//  * So the waits for these loads are counted by hand: s_waitcnt vmcnt(N) (vxb_wait_vm<N>) or a barrier that drains.  A load the
//    compiler does see only gets a stricter wait from the extra one in flight.
//  * m0: the asm sets m0 = lds_wave_base itself (s_nop 0: the SALU write -> LDS-DMA read hazard) and declares no m0 clobber.  m0 is a
//    reserved register to LLVM, which drops such a clobber with a -Winline-asm warning, so a clobber would not be honoured anyway.  What
//    makes it sound instead: in the device code (-S) of every kernel that issues these loads, each instruction that reads m0 follows its
//    own write of m0 in the same basic block (in conv_halo_bf16, flash2_fwd and flash2_bwd the only m0 readers are these loads).  A
//    kernel that starts issuing them, above all next to compiler-visible direct-to-LDS loads, has to be checked the same way.
__device__ __forceinline__ void vxb_load_lds_dwordx4(const void* base, unsigned byte_off, unsigned lds_wave_base) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(byte_off), "s"(base), "s"(lds_wave_base) : "memory");
}
__device__ __forceinline__ void vxb_load_lds_dword(const void* base, unsigned byte_off, unsigned lds_wave_base) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(byte_off), "s"(base), "s"(lds_wave_base) : "memory");
}
template <int N>
__device__ __forceinline__ void vxb_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
