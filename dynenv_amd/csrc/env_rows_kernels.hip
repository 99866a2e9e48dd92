// env_rows_kernels.hip - exact save / restore of chosen environments (dynenv_get_exact / dynenv_set_exact): every per-environment row of
// the handle, bit for bit, to and from caller-owned device memory.  Both handles use these two kernels: what they copy is the row table
// (EnvRowTable, dynenv_host.h), passed by value.  Included at the very END of dynenv_capi.hip, behind robocup_reset.hip: no kernel a
// step launches moves (rc_layout_pad, robocup_kernels.hip).
//
// One wave per listed environment (grid n), no LDS.  The rows of one array are one run of "units" (16, 8 or 4 bytes) in the blob, so
// lane l of wave iteration `it` owns unit u = 64 it + l: in the blob that is one linear segment per instruction, in the handle's array
// it is consecutive words of row u / unitsPerRow - whole field rows, each one coalesced segment (an instruction covers several short
// rows).  One pass per access width; the iterations of ALL arrays of that width form one wave-uniform sequence (a, it), and
// ENV_ROWS_BATCH of them load before the first of them stores, whatever array they belong to - most arrays are a single iteration,
// and a lone wave would otherwise pay one dependent memory round trip per array.  The loads are unconditional, so that nothing but
// address arithmetic stands between them: a lane behind the array's last unit reads that last unit again, a slot behind the
// sequence's end repeats the batch's first iteration, and only the stores are guarded.
#define ENV_ROWS_BATCH 4
typedef uint32_t env_rows_u4 __attribute__((ext_vector_type(4)));  // (native vectors: a batch's values stay where their loads put them)
typedef uint32_t env_rows_u2 __attribute__((ext_vector_type(2)));

template <bool ROWS>  // where unit u of array A lives: in the handle's rows, or in the blob (blobOff counts the header in)
DE_DEV const char* env_rows_addr(const EnvRowArr& A, unsigned u, int e, const char* blob, int wlog) {
  if (!ROWS) return blob + A.blobOff + ((size_t)u << wlog);
  const unsigned f = u / A.unitsPerRow, k = u - f * A.unitsPerRow;
  return A.base + (size_t)f * A.fieldStride + (size_t)e * A.rowBytes + ((size_t)k << wlog);
}

// the arrays whose units are V (env_rows_u4, env_rows_u2, uint32_t).  SAVE: rows -> blob; else blob -> rows.
template <bool SAVE, typename V>
DE_DEV void env_rows_copy(const EnvRowTable& T, int e, char* blob, int lane) {
  constexpr int W = sizeof(V) == 16 ? 0 : sizeof(V) == 8 ? 1 : 2, WLOG = 4 - W;
  int a = T.first[W], it = 0;  // wave-uniform cursor over (array, iteration)
  while (a < T.n) {
    V v[ENV_ROWS_BATCH];
    int sa[ENV_ROWS_BATCH], sit[ENV_ROWS_BATCH];
    const int a0 = a, it0 = it;
#pragma unroll
    for (int k = 0; k < ENV_ROWS_BATCH; ++k) {
      const bool live = a < T.n;
      sa[k] = live ? a : -1; sit[k] = it;
      const int al = live ? a : a0, il = live ? it : it0;
      const EnvRowArr& A = T.arr[al];
      unsigned u = (unsigned)il * 64u + (unsigned)lane;
      u = u < A.units ? u : A.units - 1u;
      v[k] = *(const V*)env_rows_addr<SAVE>(A, u, e, blob, WLOG);
      if (live && ++it >= (int)A.trips) { a = A.next; it = 0; }
    }
    // (every load of the batch is issued before its first store: blob and rows never alias, and left alone the compiler sinks each
    //  load to its store - one memory round trip per iteration again)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < ENV_ROWS_BATCH; ++k) {
      if (sa[k] >= 0) {
        const EnvRowArr& A = T.arr[sa[k]];
        const unsigned u = (unsigned)sit[k] * 64u + (unsigned)lane;
        if (u < A.units) *(V*)const_cast<char*>(env_rows_addr<!SAVE>(A, u, e, blob, WLOG)) = v[k];
      }
    }
  }
}

// blobs: n exact blobs T.blobBytes apart, 16-byte aligned; idx (may be nullptr: environments 0..n-1) names each blob's environment.
// An index outside [0, E) leaves its blob untouched.
extern "C" __global__ void __launch_bounds__(64)
env_rows_save_kernel(EnvRowTable T, const int* __restrict__ idx, unsigned char* __restrict__ blobs) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int e = idx ? uniform_i(idx[b]) : b;
  if ((unsigned)e >= (unsigned)T.E) return;
  char* blob = (char*)blobs + (size_t)b * T.blobBytes;
  if (lane < 4) ((uint32_t*)blob)[lane] = lane == 0 ? (uint32_t)T.tag : lane == 1 ? (uint32_t)(T.tag >> 32) : 0u;  // the header
  // the zero words that bring each array's part to a multiple of 16 bytes: at most 3 per array, one lane each, one store
  static_assert(3 * ENV_ROWS_MAX <= 64, "one lane per pad word");
  if (lane < T.nPad) *(uint32_t*)(blob + T.padAt[lane]) = 0u;
  env_rows_copy<true, env_rows_u4>(T, e, blob, lane);
  env_rows_copy<true, env_rows_u2>(T, e, blob, lane);
  env_rows_copy<true, uint32_t>(T, e, blob, lane);
}

// status (may be nullptr) int32 [n]: 0 written, 1 the blob's tag is not this table's - the environment is untouched and error bit 6 is
// raised on it -, 2 index outside [0, E).  What stands behind a valid tag is trusted.
extern "C" __global__ void __launch_bounds__(64)
env_rows_load_kernel(EnvRowTable T, const int* __restrict__ idx, const unsigned char* __restrict__ blobs, int* __restrict__ status) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int e = idx ? uniform_i(idx[b]) : b;
  if ((unsigned)e >= (unsigned)T.E) {
    if (status && lane == 0) status[b] = 2;
    return;
  }
  const char* blob = (const char*)blobs + (size_t)b * T.blobBytes;
  if (uniform_u64(*(const uint64_t*)blob) != T.tag) {
    if (lane == 0) {
      int* err = T.err + (size_t)e * T.errStride + T.errIndex;
      *err = *err | 64;
      if (status) status[b] = 1;
    }
    return;
  }
  char* src = const_cast<char*>(blob);  // (only read)
  env_rows_copy<false, env_rows_u4>(T, e, src, lane);
  env_rows_copy<false, env_rows_u2>(T, e, src, lane);
  env_rows_copy<false, uint32_t>(T, e, src, lane);
  if (status && lane == 0) status[b] = 0;
}
