// The two pieces of a fine-tuning step outside the network that walk every parameter: the regulariser lambda sum |p - p_init|
// (reference loss/parameter_loss.py:9-27) with its subgradient, and the Adam / RAdam update (torch.optim.Adam; reference
// optimizer/radam.py:8-97), each as ONE launch over a multi-tensor table.  Templated on the precision T
// (float / double) of the tensors; state and arithmetic are in T, the sum of the loss is f64.  The fold of a workgroup's sum is
// cvd_loss_common.h's.
//
// The table: K pointer arrays ptrs[K][T] (device addresses of the T tensors' first elements), counts[T], one ParamRecord per
// tensor, and the chunk list -- tensor t with n elements is cut into ceil(n / CVD_PARAM_CHUNK) chunks (chunkTensor[c],
// chunkStart[c]); a tensor of zero elements has no chunk.  Workgroups of 256 threads grid-stride over the chunk list; the grid is
// min(chunks, 2048).  A chunk whose K addresses are all 16-byte aligned (a chunk's byte length is a multiple of 16, so a tensor's
// chunks are aligned alike) moves 16 bytes per lane per access -- four f32 or two f64 -- and finishes the < 16 bytes of a
// tensor's tail one element per lane; any other chunk goes one element per lane throughout.  Both paths run the same per-element
// function, compiled without contraction: they give the same bits.
//
// k_param_l1<T>             ptrs = {p, p0, -}: a workgroup's f64 sum of |p - p0| (the difference and its magnitude in T, as the
//                           reference forms them) over its chunks goes to slab[blockIdx.x]: lanes by a shuffle tree, waves in index
//                           order.  No atomics: the value repeats bit for bit.
// k_param_l1_finish         one workgroup: total = lambda * (the slab's slots, lane-strided in index order, folded the same way).
// k_param_l1_grad<T, ACC>   ptrs = {p, p0, grad}: grad (+)= sign(p - p0) (lambda gradOut), sign(0) = 0 (torch.abs's subgradient:
//                           at the first step of fine-tuning every element is a tie); gradOut a device scalar of type T.
// k_param_step<T>           ptrs = {p, g, m, v}: the update rule the tensor's record names, p, m (exp_avg) and v (exp_avg_sq) in
//                           place.  The record's scalars are formed on the host in double, as the Python of the rule forms them,
//                           and cast to T here.
//   every rule      m = beta1 m + (1 - beta1) g,   v = beta2 v + ((1 - beta2) g) g
//   ADAM            g += gradDecay p first (gradDecay = weight_decay);  p -= step (m / (sqrt(v) / denomScale + eps))
//                   (step = lr / (1 - beta1^t), denomScale = sqrt(1 - beta2^t))
//   RADAM           p -= paramDecay p (paramDecay = weight_decay lr);  p -= step (m / (sqrt(v) + eps))   (step = step_size lr, the
//                   rectification folded into step_size; eps outside the bias correction)
//   RADAM_SGD       p -= paramDecay p;  p -= step m                       (N_sma < 5, degenerated_to_sgd)
//   MOMENTS         p stays: neither read nor written                     (N_sma < 5, not degenerated_to_sgd)
#pragma once
#include "cvd_loss_common.h"

#ifndef CVD_PARAM_CHUNK
#define CVD_PARAM_CHUNK 16384   // elements per chunk (settled by the sweep of tools/optimizer_bench.py: DESIGN.md §3.13)
#endif

namespace cvd {

constexpr int kParamChunk = CVD_PARAM_CHUNK;
static_assert(kParamChunk >= 1024 && (kParamChunk & (kParamChunk - 1)) == 0, "CVD_PARAM_CHUNK: a power of two, whole 16-byte groups");
constexpr int kParamMaxGrid = 2048;   // 256 CUs x 8 workgroups: the cap of a memory-bound grid, the rest is grid-strided
constexpr int kParamL1Arrays = 3, kParamStepArrays = 4;

enum ParamRule { PARAM_RULE_ADAM = 0, PARAM_RULE_RADAM = 1, PARAM_RULE_RADAM_SGD = 2, PARAM_RULE_MOMENTS = 3 };

struct ParamRecord {
  double beta1, omb1, beta2, omb2;   // omb = 1 - beta, in double
  double eps, gradDecay, paramDecay, step, denomScale;
  int rule, reserved;
};

struct ParamTable {
  int numTensors, numChunks;
  const unsigned long long* ptrs;   // [K][numTensors]
  const long long* counts;          // [numTensors]
  const int* chunkTensor;           // [numChunks]
  const long long* chunkStart;      // [numChunks]
  const ParamRecord* records;       // [numTensors]; k_param_step only
};

// The table holds addresses as integers: the pointers made of them are marked as global memory (global_load / global_store
// instead of the flat forms, which also wait on the LDS counter).
template <typename T>
using ParamGlobal = __attribute__((address_space(1))) T;

// 16 bytes of T
template <typename T> struct ParamVec;
template <> struct ParamVec<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct ParamVec<double> { typedef double type __attribute__((ext_vector_type(2))); };

template <typename T>
struct ParamPack {
  static constexpr int N = 16 / sizeof(T);
  typename ParamVec<T>::type v;
};

template <typename T>
__device__ __forceinline__ ParamPack<T> paramLoad(const ParamGlobal<T>* p) {
  return {*reinterpret_cast<const ParamGlobal<typename ParamVec<T>::type>*>(p)};
}
template <typename T>
__device__ __forceinline__ void paramStore(ParamGlobal<T>* p, const ParamPack<T>& q) {
  *reinterpret_cast<ParamGlobal<typename ParamVec<T>::type>*>(p) = q.v;
}

// a chunk: its tensor, its first element inside the tensor, its length
struct ParamChunk {
  int tensor, len;
  long long start;
};

__device__ __forceinline__ ParamChunk paramChunk(const ParamTable& A, int c) {
  ParamChunk k;
  k.tensor = A.chunkTensor[c];
  k.start = A.chunkStart[c];
  const long long left = A.counts[k.tensor] - k.start;
  k.len = left < kParamChunk ? static_cast<int>(left) : kParamChunk;
  return k;
}

// the address of the chunk's first element in pointer array `which`
template <typename T>
__device__ __forceinline__ ParamGlobal<T>* paramBase(const ParamTable& A, const ParamChunk& k, int which) {
  return reinterpret_cast<ParamGlobal<T>*>(A.ptrs[static_cast<size_t>(which) * A.numTensors + k.tensor]) + k.start;
}

// group(i) for the whole 16-byte groups of an aligned chunk and one(i) for the elements after them; one(i) for every element of
// any other chunk (i: the element's index in the chunk)
template <typename T, typename Group, typename One>
__device__ __forceinline__ void paramWalk(int len, bool aligned, Group&& group, One&& one) {
  constexpr int N = ParamPack<T>::N;
  if (aligned) {
    const int whole = len / N * N;
    for (int i = threadIdx.x * N; i < whole; i += kConsThreads * N) group(i);
    const int i = whole + static_cast<int>(threadIdx.x);
    if (i < len) one(i);
  } else {
    for (int i = threadIdx.x; i < len; i += kConsThreads) one(i);
  }
}

template <typename T>
__device__ __forceinline__ bool paramAligned(const ParamGlobal<T>* a, const ParamGlobal<T>* b, const ParamGlobal<T>* c = nullptr,
                                             const ParamGlobal<T>* d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

template <typename T>
inline __global__ __launch_bounds__(kConsThreads) void k_param_l1(ParamTable A, double* slab) {
#pragma clang fp contract(off)
  double acc[1] = {0.0};
  for (int c = blockIdx.x; c < A.numChunks; c += gridDim.x) {
    const ParamChunk k = paramChunk(A, c);
    const ParamGlobal<T>* p = paramBase<T>(A, k, 0);
    const ParamGlobal<T>* p0 = paramBase<T>(A, k, 1);
    paramWalk<T>(k.len, paramAligned<T>(p, p0),
                 [&](int i) {
                   const ParamPack<T> a = paramLoad(p + i), b = paramLoad(p0 + i);
#pragma unroll
                   for (int j = 0; j < ParamPack<T>::N; ++j) acc[0] += static_cast<double>(consAbs(a.v[j] - b.v[j]));
                 },
                 [&](int i) { acc[0] += static_cast<double>(consAbs(p[i] - p0[i])); });
  }
  double s;
  if (lossFoldWorkgroup(acc, s)) slab[blockIdx.x] = s;
}

inline __global__ __launch_bounds__(kConsThreads) void k_param_l1_finish(const double* slab, int nb, double lambda, double* total) {
  double acc[1] = {0.0};
  for (int j = threadIdx.x; j < nb; j += kConsThreads) acc[0] += slab[j];
  double s;
  if (lossFoldWorkgroup(acc, s)) total[0] = lambda * s;
}

template <typename T>
__device__ __forceinline__ T paramSignTimes(T p, T p0, T k) {
  const T d = p - p0;
  return d > T(0) ? k : (d < T(0) ? -k : T(0));
}

template <typename T, bool ACC>
inline __global__ __launch_bounds__(kConsThreads) void k_param_l1_grad(ParamTable A, double lambda, const T* gradOut) {
#pragma clang fp contract(off)
  const T kk = static_cast<T>(lambda) * gradOut[0];
  for (int c = blockIdx.x; c < A.numChunks; c += gridDim.x) {
    const ParamChunk k = paramChunk(A, c);
    const ParamGlobal<T>* p = paramBase<T>(A, k, 0);
    const ParamGlobal<T>* p0 = paramBase<T>(A, k, 1);
    ParamGlobal<T>* g = paramBase<T>(A, k, 2);
    paramWalk<T>(k.len, paramAligned<T>(p, p0, g),
                 [&](int i) {
                   const ParamPack<T> a = paramLoad(p + i), b = paramLoad(p0 + i);
                   ParamPack<T> q;
                   if (ACC) q = paramLoad(g + i);
#pragma unroll
                   for (int j = 0; j < ParamPack<T>::N; ++j) {
                     const T s = paramSignTimes(a.v[j], b.v[j], kk);
                     q.v[j] = ACC ? q.v[j] + s : s;
                   }
                   paramStore(g + i, q);
                 },
                 [&](int i) {
                   const T s = paramSignTimes(p[i], p0[i], kk);
                   g[i] = ACC ? g[i] + s : s;
                 });
  }
}

// a record's scalars in the compute type
template <typename T>
struct ParamScalars {
  T beta1, omb1, beta2, omb2, eps, gradDecay, paramDecay, step, denomScale;
  int rule;
};

template <typename T>
__device__ __forceinline__ ParamScalars<T> paramScalars(const ParamRecord& r) {
  return {static_cast<T>(r.beta1), static_cast<T>(r.omb1), static_cast<T>(r.beta2), static_cast<T>(r.omb2), static_cast<T>(r.eps),
          static_cast<T>(r.gradDecay), static_cast<T>(r.paramDecay), static_cast<T>(r.step), static_cast<T>(r.denomScale), r.rule};
}

// one element's update (the rule is uniform over a chunk)
template <typename T>
__device__ __forceinline__ void paramStepElement(const ParamScalars<T>& R, T& p, T g, T& m, T& v) {
#pragma clang fp contract(off)
  if (R.rule == PARAM_RULE_ADAM && R.gradDecay != T(0)) g = g + R.gradDecay * p;
  m = R.beta1 * m + R.omb1 * g;
  v = R.beta2 * v + (R.omb2 * g) * g;
  if (R.rule == PARAM_RULE_MOMENTS) return;
  if (R.rule == PARAM_RULE_ADAM) {
    p = p - R.step * (m / (consSqrt(v) / R.denomScale + R.eps));
    return;
  }
  if (R.paramDecay != T(0)) p = p - R.paramDecay * p;
  if (R.rule == PARAM_RULE_RADAM) p = p - R.step * (m / (consSqrt(v) + R.eps));
  else p = p - R.step * m;
}

template <typename T>
inline __global__ __launch_bounds__(kConsThreads) void k_param_step(ParamTable A) {
#pragma clang fp contract(off)
  for (int c = blockIdx.x; c < A.numChunks; c += gridDim.x) {
    const ParamChunk k = paramChunk(A, c);
    ParamGlobal<T>* p = paramBase<T>(A, k, 0);
    const ParamGlobal<T>* g = paramBase<T>(A, k, 1);
    ParamGlobal<T>* m = paramBase<T>(A, k, 2);
    ParamGlobal<T>* v = paramBase<T>(A, k, 3);
    const ParamScalars<T> R = paramScalars<T>(A.records[k.tensor]);
    paramWalk<T>(k.len, paramAligned<T>(p, g, m, v),
                 [&](int i) {
                   ParamPack<T> qp{}, qm = paramLoad(m + i), qv = paramLoad(v + i);
                   if (R.rule != PARAM_RULE_MOMENTS) qp = paramLoad(p + i);     // (moments only: p is neither read nor written)
                   const ParamPack<T> qg = paramLoad(g + i);
#pragma unroll
                   for (int j = 0; j < ParamPack<T>::N; ++j) {
                     T ep = qp.v[j], em = qm.v[j], ev = qv.v[j];
                     paramStepElement(R, ep, static_cast<T>(qg.v[j]), em, ev);
                     qp.v[j] = ep; qm.v[j] = em; qv.v[j] = ev;
                   }
                   if (R.rule != PARAM_RULE_MOMENTS) paramStore(p + i, qp);
                   paramStore(m + i, qm);
                   paramStore(v + i, qv);
                 },
                 [&](int i) {
                   T ep = R.rule != PARAM_RULE_MOMENTS ? p[i] : T(0), em = m[i], ev = v[i];
                   paramStepElement(R, ep, g[i], em, ev);
                   if (R.rule != PARAM_RULE_MOMENTS) p[i] = ep;
                   m[i] = em;
                   v[i] = ev;
                 });
  }
}

}  // namespace cvd
