// launch.h — the host entry points of the kernel files: every launcher and host helper a .hip file
// defines for the engine units.  The defining .hip file and the calling engine*.cpp both include this
// header, so a changed signature fails where it is compiled, not at link.  Host declarations only: it
// is not among the headers handed to hipRTC (build.py JIT_HEADERS) and none of them includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct SweepArgs;  // device.h
struct OrderArgs;  // device.h
struct LgArgs;     // logistic.h

// sweep.hip
hipError_t mmb_launch_sweep(int model, unsigned kinds, const SweepArgs& A, hipStream_t st);
hipError_t mmb_sweep_shape(int model, unsigned kinds, const SweepArgs& A, int* nwg, int* wg_per_cu);
hipError_t mmb_launch_order_chains(const OrderArgs& a, hipStream_t st);
#ifdef MMB_PHASE_PROF
void mmb_prof_dump();
#endif
#ifdef MMB_WAVE_TIMES
void mmb_wave_times_dump(int nwaves, int slots);
void mmb_wave_times_reset(hipStream_t st);
#endif

// line_amm.hip
hipError_t mmb_launch_line_amm(const SweepArgs& A, hipStream_t st);
#ifdef MMB_PHASE_PROF
void mmb_prof_dump_line();
#endif

// probe.hip
hipError_t mmb_launch_pchol_probe(int n, int d, const double* S, double* L, int32_t* pos, int32_t* info,
                                  hipStream_t st);

// logistic.hip
hipError_t mmb_lg_launch_ctl(const LgArgs& A, int start, int parity, int nbound, int fold, hipStream_t st);
hipError_t mmb_lg_launch_grad(const LgArgs& A, int parity, int nbound, int fold, hipStream_t st);

// gr.hip
hipError_t mmb_launch_gr_range(int pmon, int64_t n, int K, const double* draws, double* out,
                               hipStream_t st);
hipError_t mmb_launch_gr_stats(int pmon, int64_t n, int K, const double* draws, const int32_t* link,
                               const double* shift, double* stats, hipStream_t st);
int mmb_gr_pmax();

// summary.hip
hipError_t mmb_launch_chain_summary(int P, int64_t n, int K, int64_t kg0, int64_t bs, const double* draws,
                                    const double* shift, double* out, hipStream_t st);
hipError_t mmb_launch_order_hist(int P, int j, int64_t n, int K, const double* draws, int nt,
                                 const uint64_t* prefix, int pass, unsigned long long* counts, hipStream_t st);

// diag.hip
hipError_t mmb_launch_chain_autocov(int P, int K, int64_t i0, int64_t i1, int nlags, const int64_t* lags,
                                    const double* draws, double* out, hipStream_t st);
hipError_t mmb_launch_chain_mcse(int P, int K, int64_t i0, int64_t i1, int etype, int64_t bs, const double* draws,
                                 double* out, hipStream_t st);
hipError_t mmb_launch_change_counts(int P, int K, int64_t n, const double* draws, unsigned long long* out,
                                    hipStream_t st);
hipError_t mmb_launch_chain_cvm(int P, int K, int64_t n, int nstarts, const int64_t* starts, const double* draws,
                                double* out, hipStream_t st);
hipError_t mmb_launch_chain_mcse_from(int P, int K, const int64_t* i0s, int64_t i1, int etype, int64_t bs,
                                      const double* draws, double* out, hipStream_t st);
hipError_t mmb_launch_chain_raftery(int P, int K, int64_t n, int64_t rlo, int interp, double h, const double* draws,
                                    double* out, hipStream_t st);

// hpd.hip
uint64_t mmb_hpd_key(double x);
double mmb_hpd_unkey(uint64_t key);
int64_t mmb_hpd_tiles(int64_t n);
hipError_t mmb_launch_hpd_collect(int P, int j, int64_t n, int K, const double* draws, double lo, double hi,
                                  int64_t cap, uint64_t* below, uint64_t* above, unsigned long long* meta,
                                  hipStream_t st);
hipError_t mmb_launch_hpd_sort(uint64_t* keys, uint64_t* tmp, int64_t n, uint64_t varying, unsigned int* tilehist,
                               unsigned long long* ghist, int* in_tmp, hipStream_t st);
hipError_t mmb_launch_hpd_gap(const uint64_t* below, int64_t nb, const uint64_t* above, int64_t na, int64_t m,
                              double lo, double hi, double* part_d, long long* part_i, double* res, hipStream_t st);

// modelstats.hip
hipError_t mmb_launch_modelstats(int model, const SweepArgs& A, int nvalues, int stack, int64_t n, int K, int pmon,
                                 const double* draws, int nnodes, const int32_t* nodes, const int32_t* col,
                                 const int32_t* slot, int ncols, double* lp, hipStream_t st);
hipError_t mmb_launch_deviance(int64_t rows, int K, const double* lp, double shift, double* acc, hipStream_t st);

// predict.hip
int mmb_predict_tile(int nvalues, int stack, int P, int* S, int* RS);
hipError_t mmb_launch_predict(int model, const SweepArgs& A, int nvalues, int stack, int64_t n, int K, int pmon,
                              const double* draws, int nnodes, const int32_t* nodes, const int32_t* col0, int P,
                              const int32_t* col, const int32_t* slot, int ncols, uint64_t seed, int64_t it0,
                              int64_t thin, double* yhat, hipStream_t st);
hipError_t mmb_launch_predict_moments(int64_t rows, int K, int P, const double* yhat, const double* shift, double* acc,
                                      hipStream_t st);
