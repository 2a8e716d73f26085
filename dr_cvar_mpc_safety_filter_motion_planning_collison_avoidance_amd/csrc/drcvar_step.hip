// drcvar_step.hip — the advance kernel of the receding-horizon loop, for gfx950: one small launch
// that closes a control step of one problem (include/drcvar_mpc.h, drcvar_mpc_step_advance_f64) or
// of n_problems problems advancing in lockstep (include/drcvar_loop.h,
// drcvar_mpc_step_advance_batch_f64).  The source is compiled twice, same kernel: into the engine
// library with the single entry, and with DRCVAR_LOOP_LIBRARY into the loop library with the batch
// entry (the engine library's symbol list stays what it was).  A third build, with
// DRCVAR_LOOP_ROUTE_LIBRARY, is one of the two objects of the route library
// (include/drcvar_loop_route.h): the batch entry whose reference paths are each problem's own
// (drcvar_mpc_step_advance_batch_route_f64), and only that kernel.
//
// Reference: the caller's loop around MPCSafetyFilter.filter_trajectory, once per control step
// (core/mpc_filter.py:40-178): apply the first input, remember the optimum on a solved call
// (:154-157), build the next call's fallback inputs as _fallback does (:197-207), move the window.
// On the device one step is three launches on one stream — sampled halfspaces (device-state form,
// drcvar_sampled.hip), the QP (drcvar_mpc.hip), this kernel — that a graph captures once: every
// quantity that changes from step to step lives in device memory and is rewritten here.
//
// One workgroup of kThreads threads per problem (blockIdx.x = b; the single entry launches one);
// workgroup b works on problem b's slices of every per-problem buffer and on state[b] alone, so no
// workgroup reads what another writes and the launch needs no atomics and no ordering between
// workgroups.  Thread e owns element e of the [H, nu] input arrays
// (H nu <= DRCVAR_MPC_MAX_HORIZON DRCVAR_MPC_MAX_INPUTS = kThreads).  Everything a later store of
// this launch could overwrite (state, have_last, last_u) is read into registers first, then one
// barrier, then the stores: the order of the header's steps 1-7 is the order of the values, and no
// thread reads what another has already rewritten.  The two state words are written last by one
// lane with ordinary 8-byte stores (vector memory; the next launch on the stream reads them after
// the kernel boundary).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "drcvar_loop.h"
#ifdef DRCVAR_LOOP_ROUTE_LIBRARY
#include "drcvar_loop_route.h"
#endif
#include "drcvar_mpc.h"

namespace {

constexpr int kThreads = DRCVAR_MPC_MAX_HORIZON * DRCVAR_MPC_MAX_INPUTS;  // 256

// (the per-problem pointers: problem 0's slice; problem b's follows from the dense batch shapes)
struct StepArgs {
  const double* x_out;
  const double* u_out;
  const double* info;
  const double* x_ref_path;
  const double* u_ref_path;
  const double* disturbance;
  double* x_log;
  double* u_log;
  double* info_log;
  double* x0;
  double* x_ref_win;
  double* u_fallback;
  double* last_u;
  int32_t* have_last;
  drcvar_step_state* state;
  int64_t path_last, step_begin, log_rows;
  int H, nx, nu;
};

// c(base + k) for the pre-clamped base (see the kernel): row of a path
__device__ __forceinline__ int64_t path_row(int64_t base, int64_t k, int64_t last) {
  const int64_t r = base + k;
  return r < 0 ? 0 : (r > last ? last : r);
}

// The route form (ROUTE, drcvar_mpc_step_advance_batch_route_f64): problem b's two reference paths
// start b * stride doubles after problem 0's.  b = blockIdx.x is uniform over the workgroup, so
// the offsets are scalar arithmetic beside the other slices'; without ROUTE the strides are an
// empty struct and the body is the instructions it was.
struct NoStrides {};
struct RouteStrides {
  int64_t x_ref, u_ref;  // in doubles
};

template <bool ROUTE>
__global__ void __launch_bounds__(kThreads) step_advance_kernel(
    StepArgs a, [[maybe_unused]] std::conditional_t<ROUTE, RouteStrides, NoStrides> rs) {
  const int e = threadIdx.x;
  const int H = a.H, nx = a.nx, nu = a.nu;
  const int n_u = H * nu, n_w = (H + 1) * nx;
  {  // problem b's slices (uniform over the workgroup: scalar arithmetic)
    const int64_t b = blockIdx.x;
    a.x_out += b * n_w;
    a.u_out += b * n_u;
    a.info += b * DRCVAR_MPC_INFO_WIDTH;
    if (a.disturbance) a.disturbance += b * a.log_rows * nx;
    a.x_log += b * (a.log_rows + 1) * nx;
    a.u_log += b * a.log_rows * nu;
    a.info_log += b * a.log_rows * DRCVAR_MPC_INFO_WIDTH;
    a.x0 += b * nx;
    a.x_ref_win += b * n_w;
    a.u_fallback += b * n_u;
    a.last_u += b * n_u;
    a.have_last += b;
    a.state += b;
    if constexpr (ROUTE) {
      a.x_ref_path += b * rs.x_ref;
      a.u_ref_path += b * rs.u_ref;
    }
  }
  // ---- reads (before the barrier) ----------------------------------------------------------
  const int64_t s = a.state->step;
  const uint64_t words = a.state->stream_offset;
  // i = s - step_begin in wrapping arithmetic: in range exactly when the difference, as an
  // unsigned number, is below log_rows (any s)
  const uint64_t i = static_cast<uint64_t>(s) - static_cast<uint64_t>(a.step_begin);
  const bool logged = i < static_cast<uint64_t>(a.log_rows);
  // s' + k without overflow for any s: s held to [-(H + 2), path_last] clamps to the same rows
  const int64_t lo = -static_cast<int64_t>(H + 2);
  const int64_t base = (s < lo ? lo : (s > a.path_last ? a.path_last : s)) + 1;
  const double st = a.info[DRCVAR_MPC_INFO_STATUS];
  const bool solved = st == static_cast<double>(DRCVAR_MPC_STATUS_OPTIMAL) ||
                      st == static_cast<double>(DRCVAR_MPC_STATUS_OPTIMAL_INACCURATE);
  const bool have = solved || *a.have_last != 0;
  double keep = 0.0, next_fb = 0.0;  // last_u[e] and u_fallback[e] after this step
  if (e < n_u) {
    const int k = e / nu, j = e - k * nu;
    const double* lu = solved ? a.u_out : a.last_u;  // the fallback memory after step 3
    keep = lu[e];
    if (have && k < H - 1)
      next_fb = lu[e + nu];
    else
      next_fb = a.u_ref_path[path_row(base, k, a.path_last) * nu + j];
  }
  double x_next = 0.0;
  if (e < nx) {
    x_next = a.x_out[nx + e];
    if (a.disturbance && logged) x_next += a.disturbance[i * nx + e];
  }
  __syncthreads();
  // ---- stores --------------------------------------------------------------------------------
  if (logged) {
    if (e < nx) a.x_log[(i + 1) * nx + e] = x_next;
    if (e < nu) a.u_log[i * nu + e] = a.u_out[e];
    if (e < DRCVAR_MPC_INFO_WIDTH) a.info_log[i * DRCVAR_MPC_INFO_WIDTH + e] = a.info[e];
  }
  if (e < n_u) {
    if (solved) a.last_u[e] = keep;
    a.u_fallback[e] = next_fb;
  }
  if (e < nx) a.x0[e] = x_next;
  for (int q = e; q < n_w; q += kThreads) {
    const int k = q / nx, j = q - k * nx;
    a.x_ref_win[q] = a.x_ref_path[path_row(base, k, a.path_last) * nx + j];
  }
  if (e == 0) {
    if (solved) *a.have_last = 1;
    a.state->step = static_cast<int64_t>(static_cast<uint64_t>(s) + 1u);
    a.state->stream_offset = words + 1u;
  }
}

// the checks every entry shares, then one launch of n_problems workgroups (the strides are read by
// the route library's build alone)
int launch_step_advance(const drcvar_mpc_model* model, int64_t n_problems, const double* x_out,
                        const double* u_out, const double* info, const double* x_ref_path,
                        const double* u_ref_path, int64_t path_steps, const double* disturbance,
                        int64_t step_begin, int64_t log_rows, double* x_log, double* u_log,
                        double* info_log, double* x0, double* x_ref_win, double* u_fallback,
                        double* last_u, int32_t* have_last, drcvar_step_state* state,
                        void* stream, [[maybe_unused]] int64_t x_ref_problem_stride = 0,
                        [[maybe_unused]] int64_t u_ref_problem_stride = 0) {
  if (!model || !x_out || !u_out || !info || !x_ref_path || !u_ref_path || !x_log || !u_log ||
      !info_log || !x0 || !x_ref_win || !u_fallback || !last_u || !have_last || !state)
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (reinterpret_cast<uintptr_t>(state) % 16 != 0) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (log_rows < 0 || path_steps < 1) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (model->horizon < 1 || model->horizon > DRCVAR_MPC_MAX_HORIZON || model->n_states < 1 ||
      model->n_states > DRCVAR_MPC_MAX_STATES || model->n_inputs < 1 ||
      model->n_inputs > DRCVAR_MPC_MAX_INPUTS)
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_problems > INT32_MAX) return DRCVAR_ERR_UNSUPPORTED;  // one workgroup each: the grid's limit
  if (x_ref_problem_stride > (int64_t{1} << 40) || u_ref_problem_stride > (int64_t{1} << 40))
    return DRCVAR_ERR_UNSUPPORTED;  // (after every invalid argument: an invalid call stays invalid)
  StepArgs a{};
  a.x_out = x_out;
  a.u_out = u_out;
  a.info = info;
  a.x_ref_path = x_ref_path;
  a.u_ref_path = u_ref_path;
  a.disturbance = disturbance;
  a.x_log = x_log;
  a.u_log = u_log;
  a.info_log = info_log;
  a.x0 = x0;
  a.x_ref_win = x_ref_win;
  a.u_fallback = u_fallback;
  a.last_u = last_u;
  a.have_last = have_last;
  a.state = state;
  a.path_last = path_steps - 1;
  a.step_begin = step_begin;
  a.log_rows = log_rows;
  a.H = model->horizon;
  a.nx = model->n_states;
  a.nu = model->n_inputs;
  (void)hipGetLastError();  // clear stale errors from unrelated work
#ifdef DRCVAR_LOOP_ROUTE_LIBRARY
  hipLaunchKernelGGL(step_advance_kernel<true>, dim3(static_cast<unsigned>(n_problems)),
                     dim3(kThreads), 0, static_cast<hipStream_t>(stream), a,
                     RouteStrides{x_ref_problem_stride, u_ref_problem_stride});
#else
  hipLaunchKernelGGL(step_advance_kernel<false>, dim3(static_cast<unsigned>(n_problems)),
                     dim3(kThreads), 0, static_cast<hipStream_t>(stream), a, NoStrides{});
#endif
  return hipGetLastError() == hipSuccess ? DRCVAR_OK : DRCVAR_ERR_LAUNCH;
}

}  // namespace

#ifdef DRCVAR_LOOP_ROUTE_LIBRARY
extern "C" int drcvar_mpc_step_advance_batch_route_f64(
    const drcvar_mpc_model* model, int64_t n_problems, const double* x_out, const double* u_out,
    const double* info, const double* x_ref_path, const double* u_ref_path, int64_t path_steps,
    int64_t x_ref_problem_stride, int64_t u_ref_problem_stride, const double* disturbance,
    int64_t step_begin, int64_t log_rows, double* x_log, double* u_log, double* info_log,
    double* x0, double* x_ref_win, double* u_fallback, double* last_u, int32_t* have_last,
    drcvar_step_state* state, void* stream) {
  if (n_problems < 0) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_problems == 0) return DRCVAR_OK;  // nothing to do: no launch, no other argument is looked at
  if (x_ref_problem_stride < 0 || u_ref_problem_stride < 0) return DRCVAR_ERR_INVALID_ARGUMENT;
  return launch_step_advance(model, n_problems, x_out, u_out, info, x_ref_path, u_ref_path,
                             path_steps, disturbance, step_begin, log_rows, x_log, u_log, info_log,
                             x0, x_ref_win, u_fallback, last_u, have_last, state, stream,
                             x_ref_problem_stride, u_ref_problem_stride);
}
#elif !defined(DRCVAR_LOOP_LIBRARY)
extern "C" int drcvar_mpc_step_advance_f64(
    const drcvar_mpc_model* model, const double* x_out, const double* u_out, const double* info,
    const double* x_ref_path, const double* u_ref_path, int64_t path_steps,
    const double* disturbance, int64_t step_begin, int64_t log_rows, double* x_log, double* u_log,
    double* info_log, double* x0, double* x_ref_win, double* u_fallback, double* last_u,
    int32_t* have_last, drcvar_step_state* state, void* stream) {
  return launch_step_advance(model, 1, x_out, u_out, info, x_ref_path, u_ref_path, path_steps,
                             disturbance, step_begin, log_rows, x_log, u_log, info_log, x0,
                             x_ref_win, u_fallback, last_u, have_last, state, stream);
}
#else
extern "C" int drcvar_mpc_step_advance_batch_f64(
    const drcvar_mpc_model* model, int64_t n_problems, const double* x_out, const double* u_out,
    const double* info, const double* x_ref_path, const double* u_ref_path, int64_t path_steps,
    const double* disturbance, int64_t step_begin, int64_t log_rows, double* x_log, double* u_log,
    double* info_log, double* x0, double* x_ref_win, double* u_fallback, double* last_u,
    int32_t* have_last, drcvar_step_state* state, void* stream) {
  if (n_problems < 0) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_problems == 0) return DRCVAR_OK;  // nothing to do: no launch, no pointer is looked at
  return launch_step_advance(model, n_problems, x_out, u_out, info, x_ref_path, u_ref_path,
                             path_steps, disturbance, step_begin, log_rows, x_log, u_log, info_log,
                             x0, x_ref_win, u_fallback, last_u, have_last, state, stream);
}
#endif
