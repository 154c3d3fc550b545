// ir_jit.h — host interface of the node-IR kernel specialisation (ir_jit.cpp).
#pragma once
#include <string>
#include <vector>

#include "mamba_hip.h"

// HIP source of the sweep kernel specialised for one lowered model: its node log densities and
// block term lists as straight-line code, `kinds` = bitmask of the scheme's sampler kinds,
// `dmax` = the widest AMM block (the unrolled factorization's step count).
std::string mmb_ir_jit_source(const mmb_model_spec& spec, const mmb_ir_model& ir, unsigned kinds, int dmax);

// Code object of `src` for gfx950: from the cache, else compiled by hipRTC and cached.
// Returns 0 on success; *info says which (or why it failed).
int mmb_ir_jit_obtain(const std::string& src, std::vector<char>* code, std::string* info);

// LDS / HBM layout of a specialised kernel, shared by the generator and the engine: the AMM
// packed triangle sized to the widest AMM block (rounded to the 32-lane slot loop; the static
// kernels use 528 = tri(32)), and no candidate copy of the state (`prop`) for schemes whose
// samplers only evaluate logpdf! at one point at a time with the state restored after it (AMM,
// Gibbs closures) -- their candidate is written into the state itself (ir.h Mdl::NOPROP)
inline int mmb_ir_jit_tp(int dmax) { return ((dmax * (dmax + 1) / 2) + 31) / 32 * 32; }
inline bool mmb_ir_jit_noprop(unsigned kinds) {
  return (kinds & ~((1u << MMB_SAMPLER_AMM) | (1u << MMB_SAMPLER_GIBBS))) == 0;
}
// LDS doubles of the expression-stack area: the specialised kernel evaluates expressions in
// registers; only the lane-parallel AMWG decision (ir.h amwg_dm) keeps term weights there
inline int mmb_ir_jit_stack_dbl(unsigned kinds) { return (kinds & (1u << MMB_SAMPLER_AMWG)) ? 32 : 0; }
