// greb_derive.hip -- the derive stage (include/greb_engine.h: greb_derive_apply_dev, greb_engine_run_derived_*).
//
// What is read off an ensemble is often not linear in its records: relative humidity q / q_sat(T), ice cover as an
// indicator, a wet-bulb temperature, the Bowen ratio.  A mean, a variance, a quantile, a crossing or a regression of such a
// quantity has to be formed from each month's record BEFORE the reduction, so it is formed here, while the year's records
// [member][12][5][np] (and [member][12][13][np] of the budget) still sit in HBM, into [member][12][n_out][np] -- the layout
// every plan kernel reads.
//
//   derive_kernel<NIN>  one streaming pass.  A lane owns four consecutive points of one (member, month): it loads every
//                       record and every field some output names once (16-byte non-temporal loads, all issued
//                       before the first instruction is interpreted), walks the program and stores each output once
//                       (16-byte stores).  NIN inputs are held in registers: 4 for most programs, 26 for any.
//
// The program is a postfix program per output.  It does not fit the kernel arguments (up to 528 words), so it lies in a
// device buffer and is read through the scalar cache (a constant-address-space pointer: s_load); every lane of the launch
// walks the same words, so every branch of the interpreter is wavefront-uniform; the next word is asked for before the
// current one is carried out.  A value stack or a local file indexed at run time would land in scratch memory.  Here the
// top of the stack lives in registers and everything below it, and the four locals, in an LDS column per lane
// (col[slot][lane]: 16 bytes a lane, consecutive lanes side by side, no lane reads another's, hence no barrier; as many
// columns as the program needs, 4 KB each, so that a short program leaves the compute unit full): a run-time slot is an LDS
// address, not a register number.  The host, which has checked the program, knows the stack depth before
// every instruction and hands the kernel code = op * 8 + slot, so the device keeps no stack pointer, and an instruction
// costs at most one 16-byte LDS access per lane beside its arithmetic (SELECT: two).  Kept in registers behind a switch
// over (op, slot), the stack cost 32 register copies per instruction where the branches of the switch met
// (tests/test_derive_isa_cpu.py: no scratch, no spills).
//
// THE SEMANTICS ARE THE DEFINITION of the results (derive.reference in Python performs the same IEEE operations): one
// fp32 operation with one rounding per arithmetic op; this file is built with -ffp-contract=off (build.py: EXTRA_FLAGS)
// and without fast-math, so that nothing is fused, reassociated or replaced by an approximation, and division and square
// root are the correctly rounded expansions.  EXP, LOG and ATAN go through fp64 and round once.
#include "greb_derive.h"

namespace greb {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) DeriveWord* prog_ptr; // scalar-loadable: immutable during a launch

// ops in the numbering of include/greb_engine.h (GREB_DV_*)
enum { kState, kTerm, kField, kConst, kTee, kGet, kAdd, kSub, kMul, kDiv, kMin, kMax, kGe, kLt, kNeg, kAbs, kSqrt, kExp, kLog, kAtan,
       kSelect };
static_assert(kSelect + 1 == kDeriveOps, "the ops of include/greb_engine.h");

#define DV_EACH(F, a, b) f4{F(a.x, b.x), F(a.y, b.y), F(a.z, b.z), F(a.w, b.w)}
#define DV_EACH1(F, a) f4{F(a.x), F(a.y), F(a.z), F(a.w)}
__device__ __forceinline__ float s_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float s_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float s_ge(float a, float b) { return a >= b ? 1.f : 0.f; }
__device__ __forceinline__ float s_lt(float a, float b) { return a < b ? 1.f : 0.f; }
__device__ __forceinline__ float s_exp(float a) { return (float)exp((double)a); }
__device__ __forceinline__ float s_log(float a) { return (float)log((double)a); }
__device__ __forceinline__ float s_atan(float a) { return (float)atan((double)a); }
__device__ __forceinline__ f4 v_add(f4 a, f4 b) { return a + b; }
__device__ __forceinline__ f4 v_sub(f4 a, f4 b) { return a - b; }
__device__ __forceinline__ f4 v_mul(f4 a, f4 b) { return a * b; }
__device__ __forceinline__ f4 v_div(f4 a, f4 b) { return a / b; }
__device__ __forceinline__ f4 v_min(f4 a, f4 b) { return DV_EACH(s_min, a, b); }
__device__ __forceinline__ f4 v_max(f4 a, f4 b) { return DV_EACH(s_max, a, b); }
__device__ __forceinline__ f4 v_ge(f4 a, f4 b) { return DV_EACH(s_ge, a, b); }
__device__ __forceinline__ f4 v_lt(f4 a, f4 b) { return DV_EACH(s_lt, a, b); }
__device__ __forceinline__ f4 v_neg(f4 a) { return -a; }
__device__ __forceinline__ f4 v_abs(f4 a) { return DV_EACH1(__builtin_fabsf, a); }
__device__ __forceinline__ f4 v_sqrt(f4 a) { return DV_EACH1(__builtin_sqrtf, a); }
__device__ __forceinline__ f4 v_exp(f4 a) { return DV_EACH1(s_exp, a); }
__device__ __forceinline__ f4 v_log(f4 a) { return DV_EACH1(s_log, a); }
__device__ __forceinline__ f4 v_atan(f4 a) { return DV_EACH1(s_atan, a); }
__device__ __forceinline__ f4 v_select(f4 c, f4 a, f4 b) {
  return f4{c.x != 0.f ? a.x : b.x, c.y != 0.f ? a.y : b.y, c.z != 0.f ? a.z : b.z, c.w != 0.f ? a.w : b.w};
}

#define DV_BIN(OP, F) case OP: top = F(col[d][t], top); break;
#define DV_UN(OP, F) case OP: top = F(top); break;
#define DV_IN1(s) case s: if (s < NIN) v = in[s < NIN ? s : 0]; break;
#define DV_IN8(s) DV_IN1(s) DV_IN1(s + 1) DV_IN1(s + 2) DV_IN1(s + 3) DV_IN1(s + 4) DV_IN1(s + 5) DV_IN1(s + 6) DV_IN1(s + 7)

template <int NIN>
__global__ __launch_bounds__(kDeriveThreads) void derive_kernel(DeriveArgs a) {
  const size_t i = (size_t)blockIdx.x * kDeriveThreads + threadIdx.x; // [member][month][group of four points]
  if (i >= a.lanes) return;
  const size_t np = a.np, gp = np >> 2;
  const size_t mm = i / gp, p = 4 * (i % gp); // mm = member * 12 + month
  const float* st = a.state + mm * kDeriveStates * np + p;
  const float* bu = a.budget + mm * kDeriveTerms * np + p; // (not read where no term is named)
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  f4 in[NIN];
#pragma unroll
  for (int s = 0; s < NIN; ++s) {
    const int j = a.src[s];
    const float* q = j < kDeriveStates ? st + (size_t)j * np
                     : j < kDeriveRecords ? bu + (size_t)(j - kDeriveStates) * np
                                          : a.fields + (size_t)(j - kDeriveRecords) * np + p;
    // (a field's load carries the hint too -- one load instruction per slot; the members' re-reads of its 18 KB, close in
    // time, are served by the L2 and the Infinity Cache all the same)
    in[s] = s < a.n_in ? __builtin_nontemporal_load(reinterpret_cast<const f4*>(q)) : zero;
  }
  float* dst = a.out + mm * (size_t)a.n_out * np + p;
  const prog_ptr prog = (prog_ptr)(unsigned long long)a.prog;
  // stack slots 0 ... a.stack_cols - 1 (the deepest slot a program reaches can only be the top), then the locals it sets
  extern __shared__ f4 lds_columns[];
  f4(*col)[kDeriveThreads] = reinterpret_cast<f4(*)[kDeriveThreads]>(lds_columns);
  const int t = threadIdx.x, locals = a.stack_cols;
  f4 top = zero; // the top of the stack
  const int last = a.n_words - 1; // (a program has at least an instruction and a store)
  int next_code = prog[0].code, next_arg = prog[0].arg;
  for (int pc = 0; pc <= last; ++pc) {
    const int code = next_code, arg = next_arg;
    const int ahead = pc < last ? pc + 1 : last;
    next_code = prog[ahead].code; next_arg = prog[ahead].arg;
    const int op = code >> 3, d = code & 7; // d: the slot the result goes to; the operands are slots d ... and the top
    const int below = d > 0 ? d - 1 : 0;    // where a push puts the old top (at d = 0 nothing below is live)
    switch (op) {
      case kState: case kTerm: case kField: {
        f4 v = zero;
        switch (arg) {
          DV_IN8(0) DV_IN8(8) DV_IN8(16) DV_IN1(24) DV_IN1(25)
          default: break;
        }
        col[below][t] = top; top = v;
      } break;
      case kConst: { const float c = __int_as_float(arg); col[below][t] = top; top = f4{c, c, c, c}; } break;
      case kTee: col[locals + arg][t] = top; break;
      case kGet: { const f4 v = col[locals + arg][t]; col[below][t] = top; top = v; } break;
      DV_BIN(kAdd, v_add) DV_BIN(kSub, v_sub) DV_BIN(kMul, v_mul) DV_BIN(kDiv, v_div) DV_BIN(kMin, v_min) DV_BIN(kMax, v_max)
      DV_BIN(kGe, v_ge) DV_BIN(kLt, v_lt)
      DV_UN(kNeg, v_neg) DV_UN(kAbs, v_abs) DV_UN(kSqrt, v_sqrt) DV_UN(kExp, v_exp) DV_UN(kLog, v_log) DV_UN(kAtan, v_atan)
      case kSelect: top = v_select(col[d][t], col[d + 1][t], top); break;
      case kDeriveStore: *reinterpret_cast<f4*>(dst + (size_t)arg * np) = top; break;
      default: break;
    }
  }
}

} // namespace

hipError_t launch_derive(const DeriveArgs& a, int n_members, hipStream_t s) {
  DeriveArgs k = a;
  k.lanes = (size_t)n_members * 12 * (a.np >> 2);
  if (k.lanes == 0) return hipSuccess;
  const dim3 grid((unsigned)((k.lanes + kDeriveThreads - 1) / kDeriveThreads)), block(kDeriveThreads);
  const size_t lds = (size_t)(a.stack_cols + a.local_cols) * kDeriveThreads * sizeof(f4); // at most 11 columns: 44 KB
  if (a.n_in <= kDeriveFewInputs) hipLaunchKernelGGL(derive_kernel<kDeriveFewInputs>, grid, block, lds, s, k);
  else hipLaunchKernelGGL(derive_kernel<kDeriveInputs>, grid, block, lds, s, k);
  return hipGetLastError();
}

} // namespace greb
