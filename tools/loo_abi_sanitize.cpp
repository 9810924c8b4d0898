// Host-side argument validation of allset_loo_rows / allset_loo_supported under AddressSanitizer + UBSan, as a stand-alone program
// (nothing sanitised is loaded into Python, nothing here touches a GPU: every call below returns before a launch).  Build and run on
// the CPU from the repository root:
//
//   hipcc -std=c++17 --offload-arch=gfx950 -fno-slp-vectorize -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -fsanitize=address,undefined tools/loo_abi_sanitize.cpp allset_amd/csrc/loo.hip allset_amd/csrc/abi.hip -o tools/loo_abi_sanitize.bin
//   tools/loo_abi_sanitize.bin
//
// (the second -fsanitize is the link step's: it pulls in the sanitizer runtime.)  Exit status 0 and "loo abi: N checks passed".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/allset_hip_ext.h"

static int failures = 0, checks = 0;

static void expect(const char* what, int rc, int want, const char* needle) {
  ++checks;
  const char* msg = allset_last_error();
  const bool ok = rc == want && (needle == nullptr || strstr(msg, needle) != nullptr) && (want != ALLSET_OK || msg[0] == '\0');
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAIL %s: status %d (want %d), message \"%s\"\n", what, rc, want, msg);
  }
}

int main() {
  alignas(16) static float src[64 * 8], out[64 * 8];
  static int32_t rowptr[3] = {0, 3, 8}, col[8] = {0, 1, 2, 3, 4, 5, 6, 7}, long_seg[1] = {1};
  static float s_src[8], s_seg[2];
  const int64_t n_seg = 2, n_src = 8, nnz = 8, d = 64;

  expect("supported(64)", allset_loo_supported(64), 1, nullptr);
  expect("supported(512)", allset_loo_supported(512), 1, nullptr);
  expect("supported(0)", allset_loo_supported(0), 0, nullptr);
  expect("supported(6)", allset_loo_supported(6), 0, nullptr);
  expect("supported(516)", allset_loo_supported(516), 0, nullptr);
  expect("supported(-4)", allset_loo_supported(-4), 0, nullptr);
  expect("long threshold", allset_loo_long_threshold() > 0, 1, nullptr);

#define LOO(rp, cl, sr, lds, ss, sg, ot, ldo, ls, nl, ns, nsrc, nz, dd) \
  allset_loo_rows(rp, cl, sr, lds, ss, sg, ot, ldo, ls, nl, ns, nsrc, nz, dd, nullptr)
  // nothing to do: returns before any pointer is looked at
  expect("n_seg == 0", LOO(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, -1, 0, n_src, nnz, d), ALLSET_OK, nullptr);
  expect("nnz == 0", LOO(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, -1, n_seg, n_src, 0, d), ALLSET_OK, nullptr);
  expect("d == 0", LOO(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, -1, n_seg, n_src, nnz, 0), ALLSET_OK, nullptr);
  // sizes
  expect("negative n_seg", LOO(rowptr, col, src, d, s_src, s_seg, out, d, nullptr, -1, -1, n_src, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "negative");
  expect("negative d", LOO(rowptr, col, src, d, s_src, s_seg, out, d, nullptr, -1, n_seg, n_src, nnz, -4), ALLSET_ERR_INVALID_ARGUMENT, "negative");
  expect("nnz beyond int32", LOO(rowptr, col, src, d, s_src, s_seg, out, d, nullptr, -1, n_seg, n_src, int64_t(1) << 31, d),
         ALLSET_ERR_INVALID_ARGUMENT, "int32");
  expect("n_seg beyond int32", LOO(rowptr, col, src, d, s_src, s_seg, out, d, nullptr, -1, int64_t(1) << 40, n_src, nnz, d),
         ALLSET_ERR_INVALID_ARGUMENT, "int32");
  // widths
  expect("d = 6", LOO(rowptr, col, src, 8, s_src, s_seg, out, 8, nullptr, -1, n_seg, n_src, nnz, 6), ALLSET_ERR_UNSUPPORTED, "not built");
  expect("d = 516", LOO(rowptr, col, src, 516, s_src, s_seg, out, 516, nullptr, -1, n_seg, n_src, nnz, 516), ALLSET_ERR_UNSUPPORTED, "not built");
  // pointers
  expect("null rowptr", LOO(nullptr, col, src, d, s_src, s_seg, out, d, nullptr, -1, n_seg, n_src, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "null");
  expect("null src", LOO(rowptr, col, nullptr, d, s_src, s_seg, out, d, nullptr, -1, n_seg, n_src, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "null");
  expect("null out", LOO(rowptr, col, src, d, s_src, s_seg, nullptr, d, nullptr, -1, n_seg, n_src, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "null");
  expect("empty table", LOO(rowptr, col, src, d, s_src, s_seg, out, d, nullptr, -1, n_seg, 0, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "empty");
  expect("contiguous rows, short table", LOO(rowptr, nullptr, src, d, nullptr, s_seg, out, d, nullptr, -1, n_seg, 5, nnz, d),
         ALLSET_ERR_INVALID_ARGUMENT, "n_src >= nnz");
  // layout
  expect("lds < d", LOO(rowptr, col, src, 32, s_src, s_seg, out, d, nullptr, -1, n_seg, n_src, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "leading");
  expect("ldo < d", LOO(rowptr, col, src, d, s_src, s_seg, out, 32, nullptr, -1, n_seg, n_src, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "leading");
  expect("lds % 4", LOO(rowptr, col, src, 66, s_src, s_seg, out, d, nullptr, -1, n_seg, n_src, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "aligned");
  expect("misaligned src", LOO(rowptr, col, src + 1, d, s_src, s_seg, out, d, nullptr, -1, n_seg, n_src, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "aligned");
  expect("misaligned out", LOO(rowptr, col, src, d, s_src, s_seg, out + 2, d, nullptr, -1, n_seg, n_src, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "aligned");
  expect("out aliases src", LOO(rowptr, col, src, d, s_src, s_seg, src, d, nullptr, -1, n_seg, n_src, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "alias");
  // the long-segment list
  expect("n_long > n_seg", LOO(rowptr, col, src, d, s_src, s_seg, out, d, long_seg, 3, n_seg, n_src, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "n_long");
  expect("n_long > 0, null list", LOO(rowptr, col, src, d, s_src, s_seg, out, d, nullptr, 1, n_seg, n_src, nnz, d), ALLSET_ERR_INVALID_ARGUMENT, "long_seg");
#undef LOO
  if (failures) {
    fprintf(stderr, "loo abi: %d of %d checks FAILED\n", failures, checks);
    return 1;
  }
  printf("loo abi: %d checks passed\n", checks);
  return 0;
}
