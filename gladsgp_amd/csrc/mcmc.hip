// Metropolis sweep steps of the GPU samplers (gladsgp_amd.mcmc: GPUSampler, one chain, and
// EnsembleSampler, many), replacing SEPIA's SepiaModel.do_mcmc / tune_step_sizes sweep as
// src/model.py:225-235 drives it.
//
// A sweep is component-wise Metropolis over mcmcList (betaU row by row, lamUz, lamWs, lamWOs).
// The sampler takes the likelihood-changing updates in speculative groups of g: ONE batched
// gp_loglik evaluates update i's proposal at each of the 2^i outcomes of the group's earlier
// updates (state set 2^i - 1 + pat, pat = bit j set when update j was accepted), and the
// decisions are then taken in order.  Around each gp_loglik this file puts two kernels of one
// workgroup per chain (thread j = principal component j), for chains that share X, P, priors,
// bounds and step types and have their own buffers, a stride apart:
//   gp_mcmc_ens_prep      proposals of the group's updates (and, for the sweep's first group,
//                         the prior-only move of betaU row 0), then the Gram inputs
//                         (beta, s = 1/lamUz, delta = 1/lamWs + 1/(lamWOs LamSim)) of every
//                         state set
//   gp_mcmc_ens_decide    the accept / reject decisions in order (per GP; lamWOs once for all
//                         on the sum), state, per-GP likelihood and acceptance counters in place,
//                         and for the sweep's last group the log posterior
//   gp_mcmc_ens_step      one group's decide and the next group's prep in one launch
//   gp_mcmc_group_prep / _decide / _step   the same three for one chain: they forward to
//                         gp_mcmc_ens_* with nchains = 1 (one set of kernels serves both)
// They replace some 100 elementwise launches per group of the tensor-op form of the same sweep
// (mcmc.py _sweep_torch, kept as the host-logic reference the CPU tests run).  Arithmetic is
// op-for-op that form's (no FMA contraction), so the chains agree with it and with the oracle
// (oracle/mcmc_ref.py) fed the same uniforms.
#include "gpfit_common.h"
#include "../../include/gpfit.h"

#pragma clang fp contract(off)

namespace {

constexpr double kRhoMax = 0.999;   // rho clipped in the Beta prior (mcmc.RHO_MAX)
constexpr int kLpTerms = 2048;      // log-posterior terms computed one per thread (LDS)

struct GroupArgs {
  gp_mcmc_state S;
  int kinds[GPFIT_MCMC_MAX_GROUP];
  int g;
  int flag;            // prep: first group of the sweep; decide: last group
};

// parameter index of an update code (1..d: betaU row, d+1 lamUz, d+2 lamWs, d+3 lamWOs; 0 is
// betaU row 0)
GP_DEV int param_of(int code, int d) { return code <= d ? 0 : code - d; }

GP_DEV double log_prior(const gp_mcmc_state& S, int p, double x) {
  const double a = S.pa[p], b = S.pb[p];
  switch (S.dist[p]) {
    case GPFIT_MCMC_GAMMA:
      return (a - 1.0) * log(x) - b * x;
    case GPFIT_MCMC_BETA: {
      const double rho = fmin(exp(-x / 4.0), kRhoMax);
      return (a - 1.0) * log(rho) + (b - 1.0) * log1p(-rho);
    }
    case GPFIT_MCMC_NORMAL: {
      const double t = (x - a) / b;
      return -0.5 * (t * t);
    }
    default:
      return 0.0;
  }
}

// The device buffers of the chain a workgroup runs: gp_mcmc_state's pointers moved by chain c's
// strides.  The bodies below read every pointer from here and P, d and the priors from the
// launch's gp_mcmc_state.
struct ChainPtrs {
  double *betaU, *lamUz, *lamWs, *lamWOs, *ll;
  const double *lam, *u, *step_betaU, *step_lamUz, *step_lamWs, *step_lamWOs;
  double *acc, *lp, *scratch;
};

GP_DEV ChainPtrs chain_ptrs(const gp_mcmc_state& S, const gp_mcmc_strides& T, long long c) {
  return {S.betaU + c * T.betaU, S.lamUz + c * T.lamUz, S.lamWs + c * T.lamWs,
          S.lamWOs + c * T.lamWOs, S.ll + c * T.ll, S.lam + c * T.lam, S.u + c * T.u,
          S.step_betaU + c * T.step_betaU, S.step_lamUz + c * T.step_lamUz,
          S.step_lamWs + c * T.step_lamWs, S.step_lamWOs + c * T.step_lamWOs,
          S.acc + c * T.acc, S.lp + c * T.lp, S.scratch + c * T.scratch};
}

// current value, step and uniforms of update `code` for element j (j = 0 for lamWOs)
GP_DEV void update_refs(const ChainPtrs& Q, int P, int d, int code, int j, double*& cur,
                        double& step, double& up, double& ua) {
  const long long off = 2LL * P * code;
  if (code <= d) {
    cur = Q.betaU + (long long)code * P + j;
    step = Q.step_betaU[(long long)code * P + j];
  } else if (code == d + 1) {
    cur = Q.lamUz + j;
    step = Q.step_lamUz[j];
  } else if (code == d + 2) {
    cur = Q.lamWs + j;
    step = Q.step_lamWs[j];
  } else {
    cur = Q.lamWOs;
    step = Q.step_lamWOs[0];
    up = Q.u[off];
    ua = Q.u[off + 1];
    return;
  }
  up = Q.u[off + j];
  ua = Q.u[off + P + j];
}

// proposal of parameter p from x (mcmc.propose): candidate (x when rejected by the bounds or
// rho's range), in-bounds flag and the prior difference
GP_DEV void propose(const gp_mcmc_state& S, int p, double x, double step, double up,
                    double& cand, bool& ok, double& dlp) {
  if (S.steptype[p] == GPFIT_MCMC_STEP_BETARHO) {
    const double rho = exp(-x / 4.0) + step * (up - 0.5);
    ok = (rho > 0.0) && (rho <= 1.0);
    cand = -4.0 * log(ok ? rho : 1.0);
  } else {
    cand = x + step * (up - 0.5);
    ok = true;
  }
  ok = ok && (cand >= S.lo[p]) && (cand <= S.hi[p]);
  cand = ok ? cand : x;
  dlp = log_prior(S, p, cand) - log_prior(S, p, x);
}

GP_DEV void prep_body(const GroupArgs& A, const ChainPtrs& Q, double* __restrict__ beta,
                      double* __restrict__ s, double* __restrict__ delta) {
  const gp_mcmc_state& S = A.S;
  const int j = threadIdx.x, P = S.P, d = S.d;
  double* cand = Q.scratch;                               // [i][P]
  double* okf = Q.scratch + GPFIT_MCMC_MAX_GROUP * P;
  double* dlp = Q.scratch + 2 * GPFIT_MCMC_MAX_GROUP * P;
  // The prior-only move of betaU row 0 and the group's g proposals are independent (each reads
  // the current state of its own element only; the Gram inputs below never read row 0), so
  // thread t runs row 0's element t (t < P) or update t / P - 1's element t % P: one chain of
  // fp64 exp / log per thread instead of up to g + 1 in turn (the kernel was 9.6-10.6 us,
  // profiles/r05/r05_prof_fit2.txt).  The same arithmetic per element, so the same bits.
  for (int t = j; t < (A.g + 1) * P; t += blockDim.x) {
    const int i = t / P - 1, e = t - (t / P) * P;
    if (i < 0) {                                          // betaU row 0: prior only
      if (!A.flag) continue;
      double *cur, step, up, ua;
      update_refs(Q, P, d, 0, e, cur, step, up, ua);
      double c, dl;
      bool ok;
      propose(S, 0, *cur, step, up, c, ok, dl);
      const bool acc = ok && (log(ua) < dl);
      if (acc) *cur = c;
      Q.acc[e] += acc ? 1.0 : 0.0;
      continue;
    }
    const int code = A.kinds[i];
    if (code == d + 3 && e > 0) continue;                 // lamWOs: one element
    double *cur, step, up, ua;
    update_refs(Q, P, d, code, e, cur, step, up, ua);
    double c, dl;
    bool ok;
    propose(S, param_of(code, d), *cur, step, up, c, ok, dl);
    cand[i * P + e] = c;
    okf[i * P + e] = ok ? 1.0 : 0.0;
    dlp[i * P + e] = dl;
  }
  __syncthreads();
  if (j >= P) return;
  const double lam = Q.lam[j];
  for (int i = 0; i < A.g; ++i) {
    for (int pat = 0; pat < (1 << i); ++pat) {
      const int slot = (1 << i) - 1 + pat;
      const long long row = (long long)slot * P + j;
      double lUz = Q.lamUz[j], lWs = Q.lamWs[j], lWO = Q.lamWOs[0];
      for (int r = 1; r <= d; ++r) {
        double v = Q.betaU[(long long)r * P + j];
        for (int q = 0; q <= i; ++q)
          if ((q == i || ((pat >> q) & 1)) && A.kinds[q] == r) v = cand[q * P + j];
        beta[row * d + (r - 1)] = v;
      }
      for (int q = 0; q <= i; ++q) {
        if (!(q == i || ((pat >> q) & 1))) continue;
        const int code = A.kinds[q];
        if (code == d + 1) lUz = cand[q * P + j];
        else if (code == d + 2) lWs = cand[q * P + j];
        else if (code == d + 3) lWO = cand[q * P];
      }
      s[row] = 1.0 / lUz;
      delta[row] = 1.0 / lWs + 1.0 / (lWO * lam);
    }
  }
}

GP_DEV void decide_body(const GroupArgs& A, const ChainPtrs& Q,
                        const double* __restrict__ ll_all) {
  const gp_mcmc_state& S = A.S;
  const int j = threadIdx.x, P = S.P, d = S.d;
  const double* cand = Q.scratch;
  const double* okf = Q.scratch + GPFIT_MCMC_MAX_GROUP * P;
  const double* dlp = Q.scratch + 2 * GPFIT_MCMC_MAX_GROUP * P;
  __shared__ double sh[1024];
  __shared__ int sh_acc;
  int pat = 0;
  for (int i = 0; i < A.g; ++i) {
    const int code = A.kinds[i];
    const double lln = j < P ? ll_all[((long long)(1 << i) - 1 + pat) * P + j] : 0.0;
    bool acc = false;
    if (code == d + 3) {                       // lamWOs: one decision on the sum over GPs
      if (j < P) sh[j] = lln - Q.ll[j];
      __syncthreads();
      if (j == 0) {
        double sum = 0.0;
        for (int q = 0; q < P; ++q) sum += sh[q];
        double *cur, step, up, ua;
        update_refs(Q, P, d, code, 0, cur, step, up, ua);
        const bool a = okf[i * P] != 0.0 && (log(ua) < sum + dlp[i * P]);
        if (a) *cur = cand[i * P];
        Q.acc[(long long)code * P] += a ? 1.0 : 0.0;
        sh_acc = a;
      }
      __syncthreads();
      acc = sh_acc != 0;
      if (acc && j < P) Q.ll[j] = lln;
    } else if (j < P) {
      double *cur, step, up, ua;
      update_refs(Q, P, d, code, j, cur, step, up, ua);
      acc = okf[i * P + j] != 0.0 && (log(ua) < lln - Q.ll[j] + dlp[i * P + j]);
      if (acc) {
        *cur = cand[i * P + j];
        Q.ll[j] = lln;
      }
      Q.acc[(long long)code * P + j] += acc ? 1.0 : 0.0;
    }
    pat |= (acc ? 1 : 0) << i;
    __syncthreads();
  }
  if (!A.flag) return;
  // log posterior of the state reached (mcmc.GPUSampler.log_post).  The d + 3 prior terms of
  // each GP are independent: with room in LDS one thread per term, then thread j adds its GP's
  // terms in the serial order (same bits; d + 3 fp64 log / exp chains in turn before)
  __shared__ double terms[kLpTerms];
  const int nt = (d + 3) * P;
  if (nt <= kLpTerms) {
    for (int t = j; t < nt; t += blockDim.x) {
      const int q = t / P, e = t - q * P;
      terms[t] = q <= d ? log_prior(S, 0, Q.betaU[(long long)q * P + e])
                        : (q == d + 1 ? log_prior(S, 1, Q.lamUz[e]) : log_prior(S, 2, Q.lamWs[e]));
    }
    __syncthreads();
    if (j < P) {
      double t = Q.ll[j];
      for (int q = 0; q < d + 3; ++q) t += terms[q * P + j];
      sh[j] = t;
    }
  } else if (j < P) {
    double t = Q.ll[j];
    for (int r = 0; r <= d; ++r) t += log_prior(S, 0, Q.betaU[(long long)r * P + j]);
    t += log_prior(S, 1, Q.lamUz[j]);
    t += log_prior(S, 2, Q.lamWs[j]);
    sh[j] = t;
  }
  __syncthreads();
  if (j == 0) {
    double sum = 0.0;
    for (int q = 0; q < P; ++q) sum += sh[q];
    Q.lp[0] = sum + log_prior(S, 3, Q.lamWOs[0]);
  }
}

// The kernels: workgroup c runs the bodies on chain c's buffers (the state's pointers moved by c
// strides) and on chain c's rows of the chain-major batch, which start at c (2^g - 1) P.  No
// workgroup reads or writes another chain's memory, so a chain's results do not depend on the
// others of the launch; a lone chain is the launch of one workgroup.
GP_DEV long long chain_rows(const GroupArgs& A) {
  return (long long)blockIdx.x * ((1LL << A.g) - 1) * A.S.P;
}

__global__ __launch_bounds__(1024) void mcmc_ens_prep_kernel(GroupArgs A, gp_mcmc_strides T,
                                                             double* __restrict__ beta,
                                                             double* __restrict__ s,
                                                             double* __restrict__ delta) {
  const long long r = chain_rows(A);
  prep_body(A, chain_ptrs(A.S, T, blockIdx.x), beta + r * A.S.d, s + r, delta + r);
}

__global__ __launch_bounds__(1024) void mcmc_ens_decide_kernel(GroupArgs A, gp_mcmc_strides T,
                                                               const double* __restrict__ ll_all) {
  decide_body(A, chain_ptrs(A.S, T, blockIdx.x), ll_all + chain_rows(A));
}

// A group's decisions, then the next group's proposals and Gram inputs, in one launch (the
// barrier orders the decisions' state and scratch reads before the proposals' writes)
__global__ __launch_bounds__(1024) void mcmc_ens_step_kernel(GroupArgs D, gp_mcmc_strides T,
                                                             const double* __restrict__ ll_all,
                                                             GroupArgs A,
                                                             double* __restrict__ beta,
                                                             double* __restrict__ s,
                                                             double* __restrict__ delta) {
  decide_body(D, chain_ptrs(D.S, T, blockIdx.x), ll_all + chain_rows(D));
  __syncthreads();
  const long long r = chain_rows(A);
  prep_body(A, chain_ptrs(A.S, T, blockIdx.x), beta + r * A.S.d, s + r, delta + r);
}

// 0, or 1 when the strides are unusable: none given, or with more than one chain a negative
// stride, or one below the per-chain extent of a buffer the kernels write (chains would share
// or overlap elements they write).  One chain never uses them.
int bad_strides(const gp_mcmc_strides* T, int nchains, int P, int d) {
  if (!T) return 1;
  if (nchains == 1) return 0;
  const long long ro[] = {T->lam, T->u, T->step_betaU, T->step_lamUz, T->step_lamWs,
                          T->step_lamWOs};
  for (long long v : ro)
    if (v < 0) return 1;
  const long long written[][2] = {{T->betaU, (long long)(d + 1) * P}, {T->lamUz, P},
                                  {T->lamWs, P}, {T->lamWOs, 1}, {T->ll, P},
                                  {T->acc, (long long)(d + 4) * P}, {T->lp, 1},
                                  {T->scratch, 3LL * GPFIT_MCMC_MAX_GROUP * P}};
  for (const auto& w : written)
    if (w[0] < w[1]) return 1;
  return 0;
}

int group_args(const gp_mcmc_state* S, const int* kinds, int g, int flag, GroupArgs& A) {
  if (!S) return -1;
  if (S->P < 1 || S->P > 1024) return -2;
  if (S->d < 1 || S->d > GPFIT_MAX_DIM) return -3;
  if (g < 1 || g > GPFIT_MCMC_MAX_GROUP || !kinds) return -4;
  if (!S->betaU || !S->lamUz || !S->lamWs || !S->lamWOs || !S->ll || !S->lam || !S->u ||
      !S->step_betaU || !S->step_lamUz || !S->step_lamWs || !S->step_lamWOs || !S->acc ||
      !S->lp || !S->scratch)
    return -5;
  A.S = *S;
  for (int i = 0; i < g; ++i) {
    if (kinds[i] < 1 || kinds[i] > S->d + 3) return -6;
    A.kinds[i] = kinds[i];
  }
  for (int i = g; i < GPFIT_MCMC_MAX_GROUP; ++i) A.kinds[i] = 0;
  A.g = g;
  A.flag = flag;
  return 0;
}

// One group's argument checks in gpfit.h's order: the group itself (-1 .. -6, group_args), its
// batch pointers (-7), the chain count (-8), the strides (-9)
int check_group(const gp_mcmc_state* S, const gp_mcmc_strides* T, int nchains, const int* kinds,
                int g, int flag, bool batch_ok, GroupArgs& A) {
  const int rc = group_args(S, kinds, g, flag, A);
  if (rc) return rc;
  if (!batch_ok) return -7;
  if (nchains < 1 || nchains > GPFIT_MCMC_MAX_CHAINS) return -8;
  return bad_strides(T, nchains, S->P, S->d) ? -9 : 0;
}

// one workgroup per chain, a thread per GP rounded up to whole waves
template <typename Kernel, typename... Args>
int launch(Kernel kernel, int nchains, int P, hipStream_t stream, const Args&... args) {
  hipLaunchKernelGGL(kernel, dim3(nchains), dim3((P + 63) / 64 * 64), 0, stream, args...);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : GPFIT_ERR_HIP - (int)e;
}

}  // namespace

extern "C" int gp_mcmc_ens_prep(const gp_mcmc_state* S, const gp_mcmc_strides* strides,
                                int nchains, const int* kinds, int g, int first, double* beta,
                                double* s, double* delta, hipStream_t stream) {
  GroupArgs A;
  const int rc = check_group(S, strides, nchains, kinds, g, first, beta && s && delta, A);
  if (rc) return rc;
  return launch(mcmc_ens_prep_kernel, nchains, S->P, stream, A, *strides, beta, s, delta);
}

extern "C" int gp_mcmc_ens_decide(const gp_mcmc_state* S, const gp_mcmc_strides* strides,
                                  int nchains, const int* kinds, int g, int last,
                                  const double* ll_all, hipStream_t stream) {
  GroupArgs A;
  const int rc = check_group(S, strides, nchains, kinds, g, last, ll_all != nullptr, A);
  if (rc) return rc;
  return launch(mcmc_ens_decide_kernel, nchains, S->P, stream, A, *strides, ll_all);
}

extern "C" int gp_mcmc_ens_step(const gp_mcmc_state* S, const gp_mcmc_strides* strides,
                                int nchains, const int* kinds, int g, int last,
                                const double* ll_all, const gp_mcmc_state* S_next,
                                const int* kinds_next, int g_next, int first, double* beta,
                                double* s, double* delta, hipStream_t stream) {
  GroupArgs D, A;
  int rc = check_group(S, strides, nchains, kinds, g, last, ll_all != nullptr, D);
  if (rc) return rc;
  rc = group_args(S_next, kinds_next, g_next, first, A);
  if (rc) return rc - 10;
  if (!beta || !s || !delta) return -17;
  if (S_next->P != S->P) return -18;
  if (bad_strides(strides, nchains, S_next->P, S_next->d)) return -19;
  return launch(mcmc_ens_step_kernel, nchains, S->P, stream, D, *strides, ll_all, A, beta, s,
                delta);
}

// The single-chain entry points: the ensemble's with one chain and strides that are never read
// (-8, -9 and -19 cannot fire: bad_strides accepts any struct for one chain).
extern "C" int gp_mcmc_group_prep(const gp_mcmc_state* S, const int* kinds, int g, int first,
                                  double* beta, double* s, double* delta, hipStream_t stream) {
  const gp_mcmc_strides none = {};
  return gp_mcmc_ens_prep(S, &none, 1, kinds, g, first, beta, s, delta, stream);
}

extern "C" int gp_mcmc_group_decide(const gp_mcmc_state* S, const int* kinds, int g, int last,
                                    const double* ll_all, hipStream_t stream) {
  const gp_mcmc_strides none = {};
  return gp_mcmc_ens_decide(S, &none, 1, kinds, g, last, ll_all, stream);
}

extern "C" int gp_mcmc_group_step(const gp_mcmc_state* S, const int* kinds, int g, int last,
                                  const double* ll_all, const gp_mcmc_state* S_next,
                                  const int* kinds_next, int g_next, int first, double* beta,
                                  double* s, double* delta, hipStream_t stream) {
  const gp_mcmc_strides none = {};
  return gp_mcmc_ens_step(S, &none, 1, kinds, g, last, ll_all, S_next, kinds_next, g_next, first,
                          beta, s, delta, stream);
}
