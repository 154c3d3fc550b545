// engine_ir.cpp — the node IR on the host: validation of a lowered model, the device form of its
// expressions, the separable-AMWG tables, and the choice of the specialised kernel (ir_jit.cpp).
#include "engine.h"

#include <map>

// ---- node IR: AMWG blocks whose logpdf! separates by coordinate (lane-parallel decisions) ----
// amwg_sub! (amwg.jl:99-115) evaluates logpdf!(m, x, block) once per coordinate.  The block's
// terms (simulation.jl:77-90) are sums over node elements (logpdf_sub, distributionstruct.jl:
// 136-168); when every element's term reads at most one coordinate of the block -- through the
// node's own value or a parameter expression's VAL / VALI / VALG slot -- coordinate j's two
// evaluations differ exactly in the terms of the elements that read j, whatever the accept
// history of the other coordinates, so every coordinate's difference can be formed at once (ir.h
// amwg_dm, samplers.h amwg_lanes).  The table lists, per coordinate, the (term, element) pairs
// that read it, then the pairs that read none; an MvNormal term's sigma must read none.  The
// gather indices are data, so this is built per engine at upload, not in the JIT source.
// (VALV / DATAV index with a state value: the index node's slot, and for VALV the first slot of the
// indexed node, which names its owner; *dyn tells a caller that needs the exact slots)
void ir_expr_slots(const std::vector<int32_t>& code, const std::vector<double>& pool, int pc, int i,
                   std::vector<int>& slots, bool* dyn) {
  for (;; ++pc) {
    const int w = code[pc];
    const int op = (int)((uint32_t)w >> 24), arg = w & 0xffffff;
    if (op == MMB_IR_OP_END) return;
    if (op == MMB_IR_OP_VAL) slots.push_back(arg);
    else if (op == MMB_IR_OP_VALI) slots.push_back(arg + i);
    else if (op == MMB_IR_OP_VALG) slots.push_back(arg + (int)pool[code[++pc] + i]);
    else if (op == MMB_IR_OP_VALV || op == MMB_IR_OP_DATAV) {
      if (op == MMB_IR_OP_VALV) slots.push_back(arg);
      slots.push_back(code[++pc] + i);
      if (dyn) *dyn = true;
    }
  }
}
bool ir_sep_table(const std::vector<mmb_ir_node>& nodes, const std::vector<int32_t>& code,
                  const std::vector<double>& pool, const mmb_ir_block& IB, const mmb_block_spec& s,
                  int nvalues, std::vector<int32_t>& tab, double* epsf) {
  std::vector<int> coord((size_t)nvalues, -1);
  int d = 0;
  for (int a = 0; a < s.nnodes; ++a) {
    const mmb_ir_node& N = nodes[s.nodes[a]];
    for (int q = 0; q < N.len; ++q) coord[N.off + q] = d + q;
    d += N.len;
  }
  if (d < 2 || d > 32) return false;
  std::vector<std::vector<int32_t>> lists((size_t)d + 1);
  int nmax = 1;
  size_t total = 0;
  std::vector<int> sl;
  for (int t = 0; t < IB.nterms; ++t) {
    const mmb_ir_node& N = nodes[IB.term[t]];
    const bool iso = N.family == MMB_IR_ISONORMAL;
    if (iso) {  // sigma (at element 0) must not read the block
      sl.clear();
      bool dyn = false;
      ir_expr_slots(code, pool, N.expr[1], 0, sl, &dyn);
      if (dyn) return false;
      for (int q : sl)
        if (coord[q] >= 0) return false;
    }
    nmax = std::max(nmax, (N.len + 31) / 32);
    for (int i = 0; i < N.len; ++i) {
      sl.clear();
      if (!N.fixed) sl.push_back(N.off + i);
      bool dyn = false;
      for (int k = 0; k < (iso ? 1 : 2); ++k)
        if (N.expr[k] >= 0) ir_expr_slots(code, pool, N.expr[k], i, sl, &dyn);
      if (dyn) return false;  // a state-valued index: which coordinate the element reads is not fixed
      int c = -1;
      for (int q : sl) {
        const int cq = coord[q];
        if (cq < 0) continue;
        if (c >= 0 && c != cq) return false;  // two coordinates: not separable
        c = cq;
      }
      lists[c >= 0 ? c : d].push_back((int32_t)((t << 24) | i));
      if (++total > (1u << 16)) return false;
    }
  }
  tab.assign((size_t)d + 2, 0);
  for (int j = 0; j <= d; ++j) {
    tab[(size_t)j + 1] = tab[j] + (int32_t)lists[j].size();
  }
  for (int j = 0; j <= d; ++j) tab.insert(tab.end(), lists[j].begin(), lists[j].end());
  // rounding band: each logf is a lane partial of <= nmax element terms, a 5-level butterfly, an
  // MvNormal term's affine map and the sum over the terms, so it is within (nmax + nterms + 8) u
  // of the exact sum of its element terms' magnitudes; 8x that, rounded up to a power of two
  const int n = 8 * (nmax + IB.nterms + 8);
  int e2 = 0;
  while ((1 << e2) < n) ++e2;
  *epsf = std::ldexp(1.0, e2 - 53);
  return true;
}

// Device form of the node IR's expressions: a leaf immediately followed by a binary op
// (postfix "... x leaf op") becomes one fused word MMB_IR_FUSED + 4 (leaf - 1) + (op - ADD)
// with the leaf's argument (VALG, VALV and DATAV keep their second word; the leaves end at 8, so
// the fused opcodes end at 64 + 4 * 7 + 3 = 95, within the opcode byte): acc = acc op leaf instead of
// spill, load, reload -- the same operands in the same order, so results are bit-identical
// to the oracle, which interprets the unfused code.  Each distinct expression start is
// rewritten once (validated code: every expression ends in END); node offsets are remapped.
void ir_fuse(const std::vector<int32_t>& code, std::vector<mmb_ir_node>& nodes,
             std::vector<mmb_ir_block>& blocks, std::vector<int32_t>& out) {
  std::map<int32_t, int32_t> start;
  auto op_of = [&](size_t pc) { return (int)((uint32_t)code[pc] >> 24); };
  // every expression start: node parameters, then the Gibbs blocks' reductions and parameters
  std::vector<int32_t*> exprs;
  for (mmb_ir_node& N : nodes)
    for (int k = 0; k < 3; ++k) exprs.push_back(&N.expr[k]);
  for (mmb_ir_block& B : blocks) {
    if (B.gibbs_family == 0) continue;
    for (int r = 0; r < B.nred; ++r) exprs.push_back(&B.red_expr[r]);
    for (int k = 0; k < 2; ++k) exprs.push_back(&B.gibbs_expr[k]);
  }
  for (int32_t* ex : exprs) {
    {
      const int32_t s0 = *ex;
      if (s0 < 0) continue;
      auto it = start.find(s0);
      if (it == start.end()) {
        const int32_t ns = (int32_t)out.size();
        start[s0] = ns;
        for (size_t pc = (size_t)s0;; ++pc) {
          const int op = op_of(pc);
          out.push_back(code[pc]);
          if (op == MMB_IR_OP_END) break;
          if (op >= 1 && op < 16) {
            const bool two = op == MMB_IR_OP_VALG || op == MMB_IR_OP_VALV || op == MMB_IR_OP_DATAV;
            const size_t nx = pc + (two ? 2 : 1);
            const int bo = op_of(nx);
            if (bo >= MMB_IR_OP_ADD && bo <= MMB_IR_OP_DIV) {
              out.back() = (int32_t)(((uint32_t)(MMB_IR_FUSED + 4 * (op - 1) + (bo - MMB_IR_OP_ADD)) << 24) |
                                     ((uint32_t)code[pc] & 0xffffffu));
              if (two) out.push_back(code[pc + 1]);
              pc = nx;  // the binary op is folded in
              continue;
            }
            if (two) out.push_back(code[++pc]);
          }
        }
        it = start.find(s0);
      }
      *ex = it->second;
    }
  }
}

// Host-side validation of a node IR: every code word, slot, pool range and gather index is
// checked against the node lengths, so no kernel can address outside its LDS row or the pool.
static int ir_check_expr(const mmb_ir_model* ir, int pc, int len, int* depth, int vlim = -1) {
  // vlim: value slots the expression may read (default nvalues; a Gibbs block's parameter
  // expressions also read its reduction slots nvalues .. nvalues + nred - 1)
  if (vlim < 0) vlim = ir->nvalues;
  int sp = 0, mx = 0;
  for (int steps = 0; steps < ir->ncode + 1; ++steps, ++pc) {
    if (pc < 0 || pc >= ir->ncode) return -1;
    const int w = ir->code[pc];
    const int op = (int)((uint32_t)w >> 24), arg = w & 0xffffff;
    if (op == MMB_IR_OP_END) {
      if (sp != 1) return -1;
      *depth = std::max(*depth, mx);
      return 0;
    }
    if (op < 16) {
      switch (op) {
        case MMB_IR_OP_CONST: if (arg >= ir->nconst) return -1; break;
        case MMB_IR_OP_VAL: if (arg >= vlim) return -1; break;
        case MMB_IR_OP_VALI: if ((int64_t)arg + len > vlim) return -1; break;
        case MMB_IR_OP_VALG: {
          if (++pc >= ir->ncode) return -1;
          const int64_t w2 = ir->code[pc];
          if (w2 < 0 || w2 + len > ir->npool) return -1;
          for (int i = 0; i < len; ++i) {
            const double q = ir->pool[w2 + i];
            if (!(q >= 0.0) || q != (double)(int64_t)q || (int64_t)arg + (int64_t)q >= vlim) return -1;
          }
          break;
        }
        case MMB_IR_OP_DATA: if ((int64_t)arg + len > ir->npool) return -1; break;
        case MMB_IR_OP_DATAS: if ((int64_t)arg >= ir->npool) return -1; break;
        case MMB_IR_OP_VALV:
        case MMB_IR_OP_DATAV: {
          // x[T]: the second word is the first state slot of a sampled discrete node T of exactly
          // `len` elements, whose support lo..hi (integers, >= 1) stays inside the indexed table
          if (++pc >= ir->ncode) return -1;
          const int64_t w2 = ir->code[pc];
          const mmb_ir_node* T = nullptr;
          for (int q = 0; q < ir->nnodes; ++q) {
            const mmb_ir_node& Q = ir->nodes[q];
            if (!Q.fixed && ir_dgs_family(Q.family) && Q.off == w2 && Q.len == len) T = &Q;
          }
          if (!T || !(T->lo >= 1.0) || !(T->hi >= T->lo) || !(T->hi < 16777216.0)) return -1;
          const int64_t top = (int64_t)arg + (int64_t)T->hi - 1;
          if (top >= (op == MMB_IR_OP_VALV ? (int64_t)ir->nvalues : ir->npool)) return -1;
          break;
        }
        default: return -1;
      }
      ++sp;
      mx = std::max(mx, sp);
    } else if (op < 32) {
      if (op > MMB_IR_OP_DIV || sp < 2) return -1;
      --sp;
    } else if (op > MMB_IR_OP_ABS || sp < 1) {
      return -1;
    }
  }
  return -1;
}

static int ir_validate(const mmb_model_spec* spec, const mmb_ir_model* ir) {
  if (spec->model != MMB_MODEL_IR) return fail(nullptr, MMB_E_ARG, "spec->model must be MMB_MODEL_IR");
  if (ir->nvalues < 1 || ir->nvalues > MMB_IR_MAX_VALUES)
    return fail(nullptr, MMB_E_UNSUPPORTED, "node IR: 1 <= nvalues <= %d", MMB_IR_MAX_VALUES);
  if (ir->nnodes < 1 || !ir->nodes || ir->ncode < 1 || !ir->code || ir->npool < 0 || (ir->npool > 0 && !ir->pool) ||
      ir->nconst < 0 || (ir->nconst > 0 && !ir->consts) || ir->nmon < 0 || (ir->nmon > 0 && !ir->mon))
    return fail(nullptr, MMB_E_ARG, "node IR: missing tables");
  if (ir->npool >= (1 << 24) || ir->nconst >= (1 << 24))  // code-word operands are 24-bit
    return fail(nullptr, MMB_E_UNSUPPORTED, "node IR: pool and constant tables must hold < 2^24 entries");
  if (ir->stack < 1 || ir->stack > MMB_IR_MAX_STACK)
    return fail(nullptr, MMB_E_ARG, "node IR: stack depth must be 1..%d", MMB_IR_MAX_STACK);
  int depth = 0;
  for (int n = 0; n < ir->nnodes; ++n) {
    const mmb_ir_node& N = ir->nodes[n];
    if (N.family < MMB_IR_NORMAL || N.family > MMB_IR_DIRICHLET || N.len < 1)
      return fail(nullptr, MMB_E_ARG, "node IR: node %d has a bad family or length", n);
    if (N.family != MMB_IR_LOGICAL) {
      const int64_t end = (int64_t)N.off + N.len;
      if (N.off < 0 || end > (N.fixed ? ir->npool : (int64_t)ir->nvalues))
        return fail(nullptr, MMB_E_ARG, "node IR: node %d values out of range", n);
    }
    if (N.family == MMB_IR_POISSON && !N.fixed)  // (infinite support: no DGS)
      return fail(nullptr, MMB_E_UNSUPPORTED, "node IR: Poisson node %d must be fixed (observed)", n);
    const bool dgs = !N.fixed && ir_dgs_family(N.family);
    if (dgs) {  // a sampled discrete node: in DGS blocks or, a binary one, in BMG, BMC3, BIA or BHMC blocks, one node
                // each (create_impl), never another kind
      bool in_dgs = false;
      for (int b = 0; b < spec->nblocks; ++b)
        for (int a = 0; a < spec->blocks[b].nnodes && a < MMB_MAX_NODES_PER_BLOCK; ++a)
          if (spec->blocks[b].nodes[a] == n) {
            const int bk = spec->blocks[b].sampler;
            if (binary_kind(bk) && !ir_binary_node(N))
              return fail(nullptr, MMB_E_ARG, "node IR: %s block %d samples a Bernoulli or DiscreteUniform(0, 1) node; "
                          "discrete node %d is not binary", binary_name(bk), b, n);
            if (bk != MMB_SAMPLER_DGS && !binary_kind(bk))
              return fail(nullptr, MMB_E_ARG, "node IR: discrete node %d can be sampled by a DGS block only", n);
            in_dgs = true;
          }
      if (!in_dgs) return fail(nullptr, MMB_E_ARG, "node IR: sampled discrete node %d is in no DGS block", n);
    }
    // integer support lo..hi of at most MMB_DGS_MAX_SUPPORT values: Categorical and DiscreteUniform
    // always (their density reads it), Bernoulli and Binomial when sampled
    if (dgs || N.family == MMB_IR_CATEGORICAL || N.family == MMB_IR_DISCRETEUNIFORM) {
      const bool ints = N.lo == std::floor(N.lo) && N.hi == std::floor(N.hi) && std::fabs(N.lo) < 16777216.0;
      if (!ints || !(N.hi >= N.lo) || (dgs && N.hi - N.lo + 1.0 > (double)MMB_DGS_MAX_SUPPORT))
        return fail(nullptr, MMB_E_ARG, "node IR: discrete node %d needs an integer support of at most %d values", n,
                    MMB_DGS_MAX_SUPPORT);
      if (N.family == MMB_IR_CATEGORICAL && N.lo != 1.0)
        return fail(nullptr, MMB_E_ARG, "node IR: Categorical node %d has support 1..K", n);
      if ((N.family == MMB_IR_BINOMIAL || N.family == MMB_IR_BERNOULLI) &&
          (N.lo != 0.0 || (N.family == MMB_IR_BERNOULLI && N.hi != 1.0)))
        return fail(nullptr, MMB_E_ARG, "node IR: discrete node %d has a bad support", n);
    }
    if (N.family == MMB_IR_DIRICHLET) {
      // one Dirichlet per node, an element per lane; alpha[len] > 0 and lmnB in the pool.  A sampled one
      // is in SliceSimplex blocks only (one node each: create_impl), and in at least one
      if (N.len < 2 || N.len > MMB_SIMPLEX_MAX)
        return fail(nullptr, MMB_E_ARG, "node IR: Dirichlet node %d needs 2..%d elements", n, MMB_SIMPLEX_MAX);
      if (N.cterm < 0 || (int64_t)N.cterm + N.len + 1 > ir->npool)
        return fail(nullptr, MMB_E_ARG, "node IR: Dirichlet node %d needs alpha[len] and lmnB in the pool", n);
      for (int i = 0; i < N.len; ++i)
        if (!(ir->pool[N.cterm + i] > 0.0 && std::isfinite(ir->pool[N.cterm + i])))
          return fail(nullptr, MMB_E_ARG, "node IR: Dirichlet node %d: alpha[%d] must be positive", n, i);
      if (!std::isfinite(ir->pool[N.cterm + N.len]))
        return fail(nullptr, MMB_E_ARG, "node IR: Dirichlet node %d: lmnB is not finite", n);
      if (!N.fixed) {
        bool in_ssx = false;
        for (int b = 0; b < spec->nblocks; ++b)
          for (int a = 0; a < spec->blocks[b].nnodes && a < MMB_MAX_NODES_PER_BLOCK; ++a)
            if (spec->blocks[b].nodes[a] == n) {
              if (spec->blocks[b].sampler != MMB_SAMPLER_SLICESIMPLEX)
                return fail(nullptr, MMB_E_ARG, "node IR: Dirichlet node %d can be sampled by a SliceSimplex block only", n);
              in_ssx = true;
            }
        if (!in_ssx) return fail(nullptr, MMB_E_ARG, "node IR: sampled Dirichlet node %d is in no SliceSimplex block", n);
      }
    } else if (mmb_ir_cat_state(N.family, N.cterm) >= 0) {
      // Categorical(P): the K = hi probabilities are the state slots of one sampled Dirichlet node of length K
      const int po = mmb_ir_cat_state(N.family, N.cterm);
      bool ok = false;
      for (int q = 0; q < ir->nnodes; ++q) {
        const mmb_ir_node& Q = ir->nodes[q];
        if (!Q.fixed && Q.family == MMB_IR_DIRICHLET && Q.off == po && (double)Q.len == N.hi) ok = true;
      }
      if (!ok)
        return fail(nullptr, MMB_E_ARG, "node IR: Categorical node %d: its probabilities must be the slots of one "
                    "sampled Dirichlet node of length K", n);
    } else {  // constant table: per element; sampled Binomial (element, value); Categorical K probabilities
      int64_t nct = N.len;
      if (N.family == MMB_IR_CATEGORICAL) nct = (int64_t)N.hi;
      else if (N.family == MMB_IR_BINOMIAL && dgs) nct = (int64_t)N.len * ((int64_t)N.hi + 1);
      if ((N.family == MMB_IR_CATEGORICAL || (N.family == MMB_IR_BINOMIAL && dgs)) && N.cterm < 0)
        return fail(nullptr, MMB_E_ARG, "node IR: node %d needs its constant table", n);
      if (N.cterm >= 0 && (int64_t)N.cterm + nct > ir->npool)
        return fail(nullptr, MMB_E_ARG, "node IR: node %d constant term out of range", n);
    }
    if (N.family == MMB_IR_BINOMIAL && dgs) {
      // n is data, one DATA / DATAS word, so that the support 0..n_i of every element is known here
      const int pc = N.expr[0];
      if (pc < 0 || pc + 1 >= ir->ncode || ir->code[pc + 1] != 0)
        return fail(nullptr, MMB_E_ARG, "node IR: sampled Binomial node %d: n must be one data word", n);
      const int op = (int)((uint32_t)ir->code[pc] >> 24), arg = ir->code[pc] & 0xffffff;
      if (op != MMB_IR_OP_DATA && op != MMB_IR_OP_DATAS)
        return fail(nullptr, MMB_E_ARG, "node IR: sampled Binomial node %d: n must be one data word", n);
      for (int i = 0; i < N.len; ++i) {
        const int64_t at = (int64_t)arg + (op == MMB_IR_OP_DATA ? i : 0);
        if (at >= ir->npool) return fail(nullptr, MMB_E_ARG, "node IR: node %d parameter 0 has invalid code", n);
        const double nn = ir->pool[at];
        if (!(nn >= 0.0 && nn <= N.hi && nn == std::floor(nn)))
          return fail(nullptr, MMB_E_ARG, "node IR: sampled Binomial node %d: n[%d] must be an integer in 0..%d", n, i,
                      (int)N.hi);
      }
    }
    const int nexpr = N.family == MMB_IR_CATEGORICAL || N.family == MMB_IR_DISCRETEUNIFORM ||
                              N.family == MMB_IR_DIRICHLET ? 0
                      : N.family == MMB_IR_LOGICAL || N.family == MMB_IR_EXPONENTIAL || N.family == MMB_IR_POISSON ||
                              N.family == MMB_IR_BERNOULLI ? 1 : 2;
    for (int k = 0; k < 3; ++k) {
      if (k >= nexpr) {
        if (N.expr[k] >= 0) return fail(nullptr, MMB_E_ARG, "node IR: node %d has extra parameters", n);
        continue;
      }
      if (ir_check_expr(ir, N.expr[k], N.family == MMB_IR_ISONORMAL && k == 1 ? 1 : N.len, &depth))
        return fail(nullptr, MMB_E_ARG, "node IR: node %d parameter %d has invalid code", n, k);
    }
  }
  if (depth > ir->stack) return fail(nullptr, MMB_E_ARG, "node IR: stack depth %d exceeds %d", depth, ir->stack);
  for (int q = 0; q < ir->nmon; ++q)
    if (ir->mon[q] < 0 || ir->mon[q] >= ir->nnodes) return fail(nullptr, MMB_E_ARG, "node IR: bad monitored node");
  if (spec->nblocks < 1 || spec->nblocks > MMB_MAX_BLOCKS)
    return fail(nullptr, MMB_E_ARG, "nblocks must be in 1..%d", MMB_MAX_BLOCKS);
  for (int b = 0; b < spec->nblocks; ++b) {
    const mmb_ir_block& B = ir->blocks[b];
    const bool gibbs = spec->blocks[b].sampler == MMB_SAMPLER_GIBBS;
    if (B.nterms < (gibbs ? 0 : 1) || B.nterms > MMB_IR_MAX_TERMS)
      return fail(nullptr, MMB_E_ARG, "node IR: block %d terms", b);
    for (int t = 0; t < B.nterms; ++t)
      if (B.term[t] < 0 || B.term[t] >= ir->nnodes || ir->nodes[B.term[t]].family == MMB_IR_LOGICAL)
        return fail(nullptr, MMB_E_ARG, "node IR: block %d term %d invalid", b, t);
    if (spec->blocks[b].sampler == MMB_SAMPLER_DGS && B.term[0] != spec->blocks[b].nodes[0])
      return fail(nullptr, MMB_E_ARG, "node IR: DGS block %d: its terms are its node, then the node's targets", b);
    if (spec->blocks[b].sampler == MMB_SAMPLER_SLICESIMPLEX && B.term[0] != spec->blocks[b].nodes[0])
      return fail(nullptr, MMB_E_ARG, "node IR: SliceSimplex block %d: its terms are its node, then the node's targets", b);
    // a Dirichlet node has no sampled parent and a state-read Categorical only its P: they are terms of
    // SliceSimplex and DGS blocks alone, and only those blocks' log densities know them (ir.h elem_lp<SX>)
    if (spec->blocks[b].sampler != MMB_SAMPLER_SLICESIMPLEX && spec->blocks[b].sampler != MMB_SAMPLER_DGS)
      for (int t = 0; t < B.nterms; ++t) {
        const mmb_ir_node& Q = ir->nodes[B.term[t]];
        if (Q.family == MMB_IR_DIRICHLET || mmb_ir_cat_state(Q.family, Q.cterm) >= 0)
          return fail(nullptr, MMB_E_ARG, "node IR: block %d term %d: a Dirichlet node or a Categorical that reads one "
                      "is a term of SliceSimplex and DGS blocks only", b, t);
      }
    if (!gibbs) {
      if (B.gibbs_family != 0) return fail(nullptr, MMB_E_ARG, "node IR: block %d is not a Gibbs block", b);
      continue;
    }
    // a Gibbs closure block (ABI 10): conjugate family, reductions over <= 2^24 elements, scalar
    // parameter expressions that may read the block's reduction slots
    if (B.gibbs_family != MMB_IR_NORMAL && B.gibbs_family != MMB_IR_INVGAMMA && B.gibbs_family != MMB_IR_GAMMA)
      return fail(nullptr, MMB_E_UNSUPPORTED,
                  "node IR: Gibbs block %d must draw rand(Normal | InverseGamma | Gamma) (a lowered closure)", b);
    if (B.nred < 0 || B.nred > MMB_IR_MAX_RED) return fail(nullptr, MMB_E_ARG, "node IR: block %d reductions", b);
    for (int r = 0; r < B.nred; ++r)
      if (B.red_len[r] < 1 || B.red_len[r] >= (1 << 24) || ir_check_expr(ir, B.red_expr[r], B.red_len[r], &depth))
        return fail(nullptr, MMB_E_ARG, "node IR: block %d reduction %d has invalid code", b, r);
    for (int k = 0; k < 2; ++k)
      if (ir_check_expr(ir, B.gibbs_expr[k], 1, &depth, ir->nvalues + B.nred))
        return fail(nullptr, MMB_E_ARG, "node IR: block %d Gibbs parameter %d has invalid code", b, k);
    if (depth > ir->stack) return fail(nullptr, MMB_E_ARG, "node IR: stack depth %d exceeds %d", depth, ir->stack);
  }
  return 0;
}

// value slots of the state row: nvalues, then the widest Gibbs block's reduction results
int ir_state_len(const mmb_model_spec* spec, const mmb_ir_model* ir) {
  int nred = 0;
  for (int b = 0; b < spec->nblocks; ++b)
    if (spec->blocks[b].sampler == MMB_SAMPLER_GIBBS) nred = std::max(nred, (int)ir->blocks[b].nred);
  return ir->nvalues + nred;
}

// Sampler kinds of the scheme and its widest AMM block (the specialised kernel's parameters)
static void ir_jit_params(const mmb_model_spec* spec, const mmb_ir_model* ir, unsigned* kinds, int* dmax) {
  *kinds = 0;
  *dmax = 0;
  for (int b = 0; b < spec->nblocks; ++b) {
    const mmb_block_spec& s = spec->blocks[b];
    *kinds |= 1u << s.sampler;
    int d = 0;
    for (int a = 0; a < s.nnodes; ++a) d += std::max(0, node_dim(*spec, ir, s.nodes[a], nullptr));
    if (s.sampler == MMB_SAMPLER_AMM) *dmax = std::max(*dmax, d);
  }
  if (*dmax == 0) *dmax = Mdl<MMB_MODEL_IR>::DMAX;  // no AMM block: the factorization is not compiled
}

// The generator (ir_jit.cpp) writes no code for DGS blocks, the discrete families they sample or the
// state-indexed leaves VALV / DATAV, which only such schemes hold: it declines those schemes whole
static const char* const kJitNoDgs = "the specialised kernel declines schemes with DGS blocks: sampled discrete "
                                     "nodes and state-indexed gathers are not generated";
// Nor for SliceSimplex blocks, the Dirichlet density or a Categorical that reads its probabilities
// from the state
// Nor for the binary samplers
static const char* const kJitNoBmg = "the specialised kernel declines schemes with BMG blocks: the binary samplers "
                                     "are not generated";
static const char* const kJitNoBmc3 = "the specialised kernel declines schemes with BMC3 blocks: the binary samplers "
                                      "are not generated";
static const char* const kJitNoBia = "the specialised kernel declines schemes with BIA blocks: the binary samplers "
                                     "are not generated";
static const char* const kJitNoBhmc = "the specialised kernel declines schemes with BHMC blocks: the binary samplers "
                                      "are not generated";
static const char* const kJitNoAbc = "the specialised kernel declines schemes with ABC blocks: the ABC update "
                                     "is not generated";
static const char* const kJitNoSimplex = "the specialised kernel declines schemes with SliceSimplex blocks and "
                                         "models with a Dirichlet node or a Categorical that reads a sampled P: "
                                         "they are not generated";
// why the generator declines the scheme (null: it does not)
static const char* ir_jit_declined(unsigned kinds, const mmb_ir_model* ir) {
  if (kinds & (1u << MMB_SAMPLER_BMG)) return kJitNoBmg;
  if (kinds & (1u << MMB_SAMPLER_BMC3)) return kJitNoBmc3;
  if (kinds & (1u << MMB_SAMPLER_BIA)) return kJitNoBia;
  if (kinds & (1u << MMB_SAMPLER_BHMC)) return kJitNoBhmc;
  if (kinds & (1u << MMB_SAMPLER_ABC)) return kJitNoAbc;
  if (kinds & (1u << MMB_SAMPLER_SLICESIMPLEX)) return kJitNoSimplex;
  for (int n = 0; n < ir->nnodes; ++n)
    if (ir->nodes[n].family == MMB_IR_DIRICHLET || mmb_ir_cat_state(ir->nodes[n].family, ir->nodes[n].cterm) >= 0)
      return kJitNoSimplex;
  if (kinds & (1u << MMB_SAMPLER_DGS)) return kJitNoDgs;
  return nullptr;
}

// The specialised kernel of a node-IR engine (ir_jit.cpp); on any failure the interpreter
// kernel runs (jit_info says why).  MMB_IR_JIT=0 selects the interpreter.
static void ir_jit_setup(mmb_engine* e, const mmb_model_spec* spec, const mmb_ir_model* ir) {
  const char* env = std::getenv("MMB_IR_JIT");
  if (env && std::string(env) == "0") {
    e->jit_info = "interpreter (MMB_IR_JIT=0)";
    return;
  }
  unsigned kinds = 0;
  int dmax = 0;
  ir_jit_params(spec, ir, &kinds, &dmax);
  if (const char* why = ir_jit_declined(kinds, ir)) {
    e->jit_info = std::string("interpreter (") + why + ")";
    return;
  }
  std::vector<char> code;
  std::string info;
  if (mmb_ir_jit_obtain(mmb_ir_jit_source(*spec, *ir, kinds, dmax), &code, &info)) {
    e->jit_info = "interpreter (specialisation failed: " + info + ")";
    return;
  }
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  hipError_t st = hipSetDevice(e->device);
  if (st == hipSuccess) st = hipModuleLoadData(&mod, code.data());
  if (st == hipSuccess) st = hipModuleGetFunction(&fn, mod, "mmb_ir_jit_kernel");
  if (st != hipSuccess) {
    if (mod) (void)hipModuleUnload(mod);
    e->jit_info = std::string("interpreter (module load failed: ") + hipGetErrorString(st) + ")";
    return;
  }
  e->jit_mod = mod;
  e->jit_fn = fn;
  // the specialised kernel's layout (ir_jit.h): AMM triangle sized to the widest AMM block, no
  // candidate state copy for AMM + Gibbs schemes, no expression stack beyond AMWG's term weights
  // (set before mmb_init_chains allocates the per-chain arrays)
  e->TP = mmb_ir_jit_tp(dmax);
  e->ir_noprop = mmb_ir_jit_noprop(kinds);
  e->ir_stack_dbl = mmb_ir_jit_stack_dbl(kinds);
  e->jit_info = "specialised kernel (" + info + ")";
  int namwg = 0, nsep = 0;
  for (const BlockHost& h : e->blocks)
    if (h.spec.sampler == MMB_SAMPLER_AMWG) {
      ++namwg;
      nsep += h.sep_d != nullptr;
    }
  if (namwg) e->jit_info += "; lane-parallel AMWG blocks: " + std::to_string(nsep) + " of " + std::to_string(namwg);
}

int mmb_create_ir(const mmb_model_spec* spec, const mmb_ir_model* ir, int device, mmb_engine** out) {
  if (!spec || !ir || !out) return fail(nullptr, MMB_E_ARG, "null argument");
  int rc = ir_validate(spec, ir);
  if (rc) return rc;
  rc = create_impl(spec, ir, device, out);
  if (rc) return rc;
  ir_jit_setup(*out, spec, ir);
  if ((*out)->ssx_kmax > 0) {
    // SliceSimplex schemes run the interpreter with the vertex rows appended to each chain's LDS
    // (fill_args): four chains per 128-thread workgroup must fit the 64 KiB of a launch
    const mmb_engine* e = *out;
    const int G = Mdl<MMB_MODEL_IR>::G;
    const int64_t per_chain = ((e->kinds & (1u << MMB_SAMPLER_AMM)) ? e->TP + 4 * Mdl<MMB_MODEL_IR>::DP + 2 : 0) +
                              2 * (int64_t)e->VS + (int64_t)(e->ir_stack + 1) * G + (int64_t)e->ssx_kmax * G;
    if (per_chain * (128 / G) * (int64_t)sizeof(double) > 65536) {
      mmb_destroy(*out);
      *out = nullptr;
      return fail(nullptr, MMB_E_UNSUPPORTED, "node IR: the scheme's LDS (%lld doubles per chain with the SliceSimplex "
                  "vertex rows) exceeds a workgroup's 64 KiB", (long long)per_chain);
    }
  }
  return 0;
}

int mmb_ir_jit_prebuild(const mmb_model_spec* spec, const mmb_ir_model* ir, char* info, int64_t n) {
  if (!spec || !ir) return fail(nullptr, MMB_E_ARG, "null argument");
  int rc = ir_validate(spec, ir);
  if (rc) return rc;
  unsigned kinds = 0;
  int dmax = 0;
  ir_jit_params(spec, ir, &kinds, &dmax);
  if (const char* why = ir_jit_declined(kinds, ir)) {
    if (info && n > 0) snprintf(info, (size_t)n, "%s", why);
    return fail(nullptr, MMB_E_UNSUPPORTED, "%s", why);
  }
  std::vector<char> code;
  std::string msg;
  rc = mmb_ir_jit_obtain(mmb_ir_jit_source(*spec, *ir, kinds, dmax), &code, &msg);
  if (info && n > 0) snprintf(info, (size_t)n, "%s", msg.c_str());
  return rc ? fail(nullptr, MMB_E_UNSUPPORTED, "%s", msg.c_str()) : 0;
}

int mmb_ir_jit_source_text(const mmb_model_spec* spec, const mmb_ir_model* ir, char* buf, int64_t n) {
  if (!spec || !ir) return fail(nullptr, MMB_E_ARG, "null argument");
  int rc = ir_validate(spec, ir);
  if (rc) return rc;
  unsigned kinds = 0;
  int dmax = 0;
  ir_jit_params(spec, ir, &kinds, &dmax);
  if (const char* why = ir_jit_declined(kinds, ir)) return fail(nullptr, MMB_E_UNSUPPORTED, "%s", why);
  const std::string src = mmb_ir_jit_source(*spec, *ir, kinds, dmax);
  if (buf && n > 0) snprintf(buf, (size_t)n, "%s", src.c_str());
  return (int)std::min<size_t>(src.size(), (size_t)INT32_MAX);
}

int mmb_ir_jit_info(const mmb_engine* e, char* buf, int64_t n) {
  if (!e) return fail(nullptr, MMB_E_ARG, "null argument");
  if (buf && n > 0) snprintf(buf, (size_t)n, "%s", e->model == MMB_MODEL_IR ? e->jit_info.c_str() : "not a node-IR engine");
  return e->jit_fn ? 1 : 0;
}
