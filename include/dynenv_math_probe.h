/* dynenv_math_probe.h — one row of every routine of dynenv_math.h, for the tests that hold the header to its claim: the same bits on
 * gfx950 and on the host.  The row is written ONCE, here: the two device translation units (dynenv_capi.hip, -O3; driving_tu.hip, -Os)
 * wrap dm_probe_wave in a kernel each, so every unit's own `static` copies of the out-of-line wrappers of csrc/dev_common.h get
 * called, and oracle/oracle_api.c runs dm_probe_row on the host.  tests/detmath_common.py names the columns and holds the
 * independent references; tests/test_detmath.py checks the host side against them, tests/test_gpu_detmath.py the device.
 *
 * Input row: a, b, c, d (DM_PROBE_NIN doubles).  Output row: DM_PROBE_NOUT doubles, in the order of the stores below.  Integer results
 * are converted exactly; Philox's four words travel as the bit patterns of two doubles.
 *
 * Under hipcc this header needs csrc/dev_common.h in front of it. */
#ifndef DYNENV_MATH_PROBE_H
#define DYNENV_MATH_PROBE_H

#include "dynenv_math.h"

#define DM_PROBE_NIN 4
#define DM_PROBE_NOUT 29

#if defined(__HIPCC__)
#define DMP_FN __device__ __forceinline__
/* the device's variants: the out-of-line wrappers as the kernels call them, dev_atan2_t with its table in LDS at byte address `tab` */
#define DMP_SINCOS(x, ps, pc) do { const DevSC q_ = dev_sincos(x); *(ps) = q_.s; *(pc) = q_.c; } while (0)
#define DMP_SINCOS_INL(x, ps, pc) do { const DevSC q_ = dev_sincos_inl(x); *(ps) = q_.s; *(pc) = q_.c; } while (0)
#define DMP_SINCOS_V(x, ps, pc) do { const DevSC q_ = dev_sincos_v(x); *(ps) = q_.s; *(pc) = q_.c; } while (0)
#define DMP_ATAN2(y, x) dev_atan2(y, x)
#define DMP_ATAN2_T(y, x, tab) dev_atan2_t(y, x, tab)
#else
#define DMP_FN static inline
/* the host's side of the same columns: what each device variant claims to be */
#define DMP_SINCOS(x, ps, pc) dm_sincos(x, ps, pc)
#define DMP_SINCOS_INL(x, ps, pc) dm_sincos(x, ps, pc)
#define DMP_SINCOS_V(x, ps, pc) dm_sincos_f(x, ps, pc)
#define DMP_ATAN2(y, x) dm_atan2(y, x)
#define DMP_ATAN2_T(y, x, tab) ((void)(tab), dm_atan2(y, x))
#endif

DMP_FN uint64_t dmp_bits(double x) {
  union { double d; uint64_t u; } q;
  q.d = x;
  return q.u;
}
DMP_FN double dmp_double(uint64_t u) {
  union { double d; uint64_t u; } q;
  q.u = u;
  return q.d;
}

DMP_FN void dm_probe_row(const double* in, double* out, int tab) {
  const double a = in[0], b = in[1], c = in[2], d = in[3];
  /* the four words of (a, b): Philox's counter, and the operands of the integer routines */
  const uint32_t u0 = (uint32_t)dmp_bits(a), u1 = (uint32_t)(dmp_bits(a) >> 32);
  const uint32_t u2 = (uint32_t)dmp_bits(b), u3 = (uint32_t)(dmp_bits(b) >> 32);
  /* dm_powi's exponent: (int)b where that is defined and the loop short, else 0 */
  const int n = (b >= 0.0 && b <= 4096.0) ? (int)b : 0;
  /* dm_randint's range from the words of b, masked so that hi - lo + 1 never overflows: lo in [-2^19, 2^19), hi - lo in [0, 2^30) */
  const int32_t lo = (int32_t)(u2 & 0xFFFFFu) - (1 << 19), hi = lo + (int32_t)(u3 & 0x3FFFFFFFu);
  double s, co;
  DMP_SINCOS(a, &s, &co);
  out[0] = s; out[1] = co;
  DMP_SINCOS_INL(a, &s, &co);
  out[2] = s; out[3] = co;
  DMP_SINCOS_V(a, &s, &co);
  out[4] = s; out[5] = co;
  out[6] = DMP_ATAN2(b, a);
  out[7] = DMP_ATAN2_T(b, a, tab);
  out[8] = dm_atan(a);
  out[9] = dm_sqrt(dm_abs(a));
  out[10] = a / b;
  out[11] = dm_rint(a);
  out[12] = dm_fma(a, b, c);
  out[13] = dms_dot(a, b, c, d);
  out[14] = dms_cross(a, b, c, d);
  out[15] = dms_point_vx(a, b, c);
  out[16] = dms_point_vy(a, b, c);
  out[17] = dms_rotate_x(a, b, c, d);
  out[18] = dms_rotate_y(a, b, c, d);
  out[19] = dms_xform_x(a, b, c, d, c);
  out[20] = dms_xform_y(a, b, c, d, d);
  out[21] = dms_k_scalar(a, b, c, d, b, a);
  out[22] = dms_acc_clamp0(a, b, c);
  out[23] = dm_powi(a, n);
  {
    const dm_u32x4 r = dm_philox((uint32_t)dmp_bits(c), (uint32_t)dmp_bits(d), u0, u1, u2, u3); /* key: the low words of c and d */
    out[24] = dmp_double((uint64_t)r.v[0] | ((uint64_t)r.v[1] << 32));
    out[25] = dmp_double((uint64_t)r.v[2] | ((uint64_t)r.v[3] << 32));
  }
  out[26] = dm_unit(u0);
  out[27] = dm_unit(u1);
  out[28] = (double)dm_randint(u0, lo, hi);
}

#if defined(__HIPCC__)
/* The body of a unit's probe kernel.  The block is the vision kernels' own: 64 threads, one wave, the arctangent table in LDS filled by
 * DEV_ATAN_TAB_INIT and made visible by a barrier, its row address computed per lane inside dev_atan2_t.  Row i = block * 64 + lane;
 * the lanes behind row n - 1 leave before the calls, which then run with a partial exec mask. */
DMP_FN void dm_probe_wave(const double* __restrict__ in, int n, double* __restrict__ out) {
  __shared__ alignas(16) double atanTabLds[30];
  const int lane = (int)threadIdx.x;
  DEV_ATAN_TAB_INIT(atanTabLds, lane);
  const int atanTab = dev_lds_addr(atanTabLds);
  __syncthreads();
  const long long i = (long long)blockIdx.x * DE_WAVE + lane;
  if (i < n) dm_probe_row(in + (size_t)i * DM_PROBE_NIN, out + (size_t)i * DM_PROBE_NOUT, atanTab);
}
#endif

#endif /* DYNENV_MATH_PROBE_H */
