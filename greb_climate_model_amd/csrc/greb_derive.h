// greb_derive.h -- host interface of the derive stage (greb_derive.hip): a model year of state records, and of budget
// records where the program names a term, turned into per-point expressions of them, record by record.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace greb {

constexpr int kDeriveThreads = 256;
constexpr int kDeriveStates = 5;     // GREB_NVAR_OUT
constexpr int kDeriveTerms = 13;     // GREB_NBUDGET
constexpr int kDeriveRecords = kDeriveStates + kDeriveTerms; // record j < 5: state j, else term j - 5
constexpr int kDeriveMaxOut = 16;    // GREB_MAX_RECORD_VARS
constexpr int kDeriveMaxIns = 64;    // GREB_DERIVE_MAX_INS
constexpr int kDeriveMaxTotal = 512; // GREB_DERIVE_MAX_TOTAL
constexpr int kDeriveMaxStack = 8;   // GREB_DERIVE_MAX_STACK
constexpr int kDeriveMaxLocals = 4;  // GREB_DERIVE_MAX_LOCALS
constexpr int kDeriveMaxFields = 8;  // GREB_DERIVE_MAX_FIELDS
constexpr int kDeriveOps = 21;       // GREB_DV_STATE ... GREB_DV_SELECT
constexpr int kDeriveStore = kDeriveOps; // the device's own op behind them: stack slot 0 is output `arg`
constexpr int kDeriveInputs = kDeriveRecords + kDeriveMaxFields; // input j < 18: record j, else field j - 18
constexpr int kDeriveFewInputs = 4;  // the instantiation most programs take: at most four inputs in registers

// The program as the kernel walks it.  The host has validated it and knows the stack depth before every instruction,
// so the device keeps no stack pointer: code = op * 8 + d, d the stack slot the instruction's result goes to (binary:
// its operands are slots d and d + 1; SELECT: d, d + 1, d + 2; TEE: the slot copied), the highest of them being the top.  arg: STATE, TERM and FIELD the slot
// of the input among the loaded ones, CONST the value's bits, TEE and GET the local, the store the output.
struct DeriveWord { int32_t code, arg; };

struct DeriveArgs {
  const DeriveWord* prog; // device memory, n_words words: each output's instructions, then its store
  const float* fields;    // device memory [n_fields][np], or null
  const float* state;     // [n_members][12][5][np]
  const float* budget;    // [n_members][12][13][np], or null when no term is named
  float* out;             // [n_members][12][n_out][np]
  size_t np, lanes;
  int n_words, n_out, n_in;
  int stack_cols, local_cols; // LDS columns (4 KB a workgroup each): the stack below its top, 1 ... 7, and the locals set, 0 ... 4
  unsigned char src[kDeriveInputs]; // the inputs loaded, ascending: src[s] is what slot s holds
};

// np % 4 == 0, every pointer 16-byte aligned
hipError_t launch_derive(const DeriveArgs& a, int n_members, hipStream_t s);

} // namespace greb
