// Per-point PCA of k-point neighbourhoods: the device side of PCAComputePointwise (reference:
// core/data_transform/features.py:307-329 `batch_pca` applied per chunk at :455-470, which runs `symeig` on the CPU).
//
// Per query point: mean of the k neighbour positions, covariance of the centred positions divided by k, eigenvalues
// ascending (negative values clamped to 0) and unit eigenvectors as rows [v0 | v1 | v2] (the reference's
// evec.transpose(2, 1).flatten(1)), so the first three values are the normal.
//
// Numerics: one pass over the neighbours accumulates, in fp64, the sums of d = p - p0 and of d d^T with p0 the first
// neighbour (a point of the neighbourhood, so |d| stays within its diameter); cov = (S_dd - s_d s_d^T / k) / k.  The
// cancellation of that difference costs ~1e-16 |d|^2 absolute, far below the fp32 output.  The symmetric 3 x 3
// problem is solved in fp64 by a fixed number of cyclic Jacobi sweeps: convergence is quadratic and 4 sweeps reach
// fp64 rounding on every neighbourhood shape (planar, collinear, isotropic); repeated and zero eigenvalues need no
// special case (a zero off-diagonal entry is not rotated, so a zero covariance keeps the identity).
#include "dva_common.h"

namespace dva {

constexpr int PCA_TPB = 64;        // one wavefront per block: the block's neighbour rows are staged in LDS
constexpr int PCA_KMAX = 128;
constexpr int PCA_SWEEPS = 6;

// rotate the (P, Q) plane so that a[P][Q] = 0 (a' = J^T a J, v' = v J)
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
  constexpr int R = 3 - P - Q;
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  // smaller root of t^2 + 2 theta t - 1 = 0; |theta| huge (apq negligible): t ~ 1 / (2 theta)
  double t = fabs(theta) < 1e150 ? 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0)) : 0.5 / fabs(theta);
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[P][P] -= t * apq;
  a[Q][Q] += t * apq;
  a[P][Q] = a[Q][P] = 0.0;
  const double arp = a[R][P], arq = a[R][Q];
  a[R][P] = a[P][R] = c * arp - s * arq;
  a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double vip = v[i][P], viq = v[i][Q];
    v[i][P] = c * vip - s * viq;
    v[i][Q] = s * vip + c * viq;
  }
}

__global__ __launch_bounds__(PCA_TPB) void pointwise_pca_kernel(const float* __restrict__ xyz, int64_t n_search,
                                                                 const int32_t* __restrict__ nbr, int64_t n, int k,
                                                                 float* __restrict__ evals,
                                                                 float* __restrict__ evecs) {
  extern __shared__ int32_t s_nbr[];      // [PCA_TPB][k | 1]: an odd row stride keeps the row reads conflict free
  const int t = threadIdx.x;
  const int ks = k | 1;
  for (int64_t base = blockIdx.x * (int64_t)PCA_TPB; base < n; base += (int64_t)gridDim.x * PCA_TPB) {
    const int rows = (int)(n - base < PCA_TPB ? n - base : PCA_TPB);
    const int32_t* src = nbr + base * k;
    __syncthreads();                      // the previous tile is consumed
    for (int e = t; e < rows * k; e += PCA_TPB) {   // coalesced copy of the block's rows
      const int r = e / k;
      s_nbr[r * ks + (e - r * k)] = src[e];
    }
    __syncthreads();
    if (t >= rows) continue;
    const int32_t* row = s_nbr + t * ks;
    // an index outside the search cloud invalidates the neighbourhood (NaN rule below) instead of being read
    bool bad = false;
    float x0 = 0.f, y0 = 0.f, z0 = 0.f;
    {
      const int32_t j = row[0];
      if ((uint32_t)j < (uint64_t)n_search) {
        x0 = xyz[3 * (int64_t)j]; y0 = xyz[3 * (int64_t)j + 1]; z0 = xyz[3 * (int64_t)j + 2];
      } else {
        bad = true;
      }
    }
    double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, syy = 0.0, szz = 0.0, sxy = 0.0, sxz = 0.0, syz = 0.0;
    for (int m = 0; m < k; ++m) {
      const int32_t j = row[m];
      if ((uint32_t)j >= (uint64_t)n_search) { bad = true; continue; }
      const double dx = (double)xyz[3 * (int64_t)j] - (double)x0;
      const double dy = (double)xyz[3 * (int64_t)j + 1] - (double)y0;
      const double dz = (double)xyz[3 * (int64_t)j + 2] - (double)z0;
      sx += dx; sy += dy; sz += dz;
      sxx += dx * dx; syy += dy * dy; szz += dz * dz;
      sxy += dx * dy; sxz += dx * dz; syz += dy * dz;
    }
    const double inv_k = 1.0 / (double)k;
    double a[3][3];
    a[0][0] = (sxx - sx * sx * inv_k) * inv_k;
    a[1][1] = (syy - sy * sy * inv_k) * inv_k;
    a[2][2] = (szz - sz * sz * inv_k) * inv_k;
    a[0][1] = a[1][0] = (sxy - sx * sy * inv_k) * inv_k;
    a[0][2] = a[2][0] = (sxz - sx * sz * inv_k) * inv_k;
    a[1][2] = a[2][1] = (syz - sy * sz * inv_k) * inv_k;
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    double w[3];
    const bool nan = bad || isnan(a[0][0]) || isnan(a[1][1]) || isnan(a[2][2]) || isnan(a[0][1]) ||
                     isnan(a[0][2]) || isnan(a[1][2]);
    if (nan) {                            // features.py:320-323: equal eigenvalues 1 and the identity
      w[0] = w[1] = w[2] = 1.0;
    } else {
#pragma unroll
      for (int sweep = 0; sweep < PCA_SWEEPS; ++sweep) {
        jacobi_rotate<0, 1>(a, v);
        jacobi_rotate<0, 2>(a, v);
        jacobi_rotate<1, 2>(a, v);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) w[c] = a[c][c] > 0.0 ? a[c][c] : 0.0;   // clamps rounding below 0 (and -0)
    }
    // ascending eigenvalues; equal ones keep their column order
    int o0 = 0, o1 = 1, o2 = 2, tmp;
    if (w[o0] > w[o1]) { tmp = o0; o0 = o1; o1 = tmp; }
    if (w[o1] > w[o2]) { tmp = o1; o1 = o2; o2 = tmp; }
    if (w[o0] > w[o1]) { tmp = o0; o0 = o1; o1 = tmp; }
    const int64_t i = base + t;
    const int ord[3] = {o0, o1, o2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int oc = ord[c];
      const float e0 = (float)(oc == 0 ? v[0][0] : (oc == 1 ? v[0][1] : v[0][2]));
      const float e1 = (float)(oc == 0 ? v[1][0] : (oc == 1 ? v[1][1] : v[1][2]));
      const float e2 = (float)(oc == 0 ? v[2][0] : (oc == 1 ? v[2][1] : v[2][2]));
      const double we = oc == 0 ? w[0] : (oc == 1 ? w[1] : w[2]);
      // sign, decided on the fp32 output: its component of largest magnitude (the first of equal ones) is positive
      float big = e0;
      if (fabsf(e1) > fabsf(big)) big = e1;
      if (fabsf(e2) > fabsf(big)) big = e2;
      const float sg = big < 0.f ? -1.f : 1.f;
      evals[3 * i + c] = (float)we;
      evecs[9 * i + 3 * c] = sg * e0;
      evecs[9 * i + 3 * c + 1] = sg * e1;
      evecs[9 * i + 3 * c + 2] = sg * e2;
    }
  }
}

}  // namespace dva

using namespace dva;

extern "C" {

int dva_pointwise_pca(const float* search_xyz, int64_t n_search, const int32_t* neighbors, int64_t n_query,
                      int32_t k, float* eigenvalues, float* eigenvectors, void* stream) {
  if (n_query < 0 || n_search < 0 || k <= 0 || k > PCA_KMAX || n_search < k) return DVA_ERR_INVALID;
  if (n_query > 0x7fffffffLL || n_search > 0x7fffffffLL) return DVA_ERR_UNSUPPORTED;
  if (n_query == 0) return DVA_OK;
  if (!search_xyz || !neighbors || !eigenvalues || !eigenvectors) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  int64_t blocks = (n_query + PCA_TPB - 1) / PCA_TPB;
  if (blocks > 256 * 32) blocks = 256 * 32;
  const size_t lds = (size_t)PCA_TPB * (size_t)(k | 1) * sizeof(int32_t);
  hipLaunchKernelGGL(pointwise_pca_kernel, dim3((int)blocks), dim3(PCA_TPB), lds, s, search_xyz, n_search, neighbors,
                     n_query, (int)k, eigenvalues, eigenvectors);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
