// Control for tests/test_isa_hazards.py: compiled for gfx950 (device code only) into a temporary directory and
// disassembled there; never linked into the library and never launched.  hazard_asm_pack feeds a v_cvt_pk_bf16_f32
// written as inline asm straight into an MFMA, the form pack_bf16x2 had before DESIGN section 24 (hipcc's hazard
// recognizer does not look into the string, so the MFMA sits one state behind the write); hazard_visible_pack is the
// same kernel with the conversion the compiler sees, today's pack_bf16x2, which hipcc pads to two states.
#include <hip/hip_runtime.h>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <bool ASM>
__device__ __forceinline__ unsigned pack(float a, float b) {
  if constexpr (ASM) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  } else {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
  }
}

template <bool ASM>
__device__ __forceinline__ void body(const float* x, const u32x4* w, f32x4* out) {
  const int lane = threadIdx.x;
  const u32x4 b = w[lane];
  const f32x4 lo = reinterpret_cast<const f32x4*>(x)[2 * lane], hi = reinterpret_cast<const f32x4*>(x)[2 * lane + 1];
  const u32x4 a = {pack<ASM>(lo[0], lo[1]), pack<ASM>(lo[2], lo[3]), pack<ASM>(hi[0], hi[1]), pack<ASM>(hi[2], hi[3])};
  out[lane] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                      f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
}

extern "C" __global__ void hazard_asm_pack(const float* x, const u32x4* w, f32x4* out) { body<true>(x, w, out); }
extern "C" __global__ void hazard_visible_pack(const float* x, const u32x4* w, f32x4* out) { body<false>(x, w, out); }
