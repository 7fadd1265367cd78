// Host-side argument checks of the permuted-row entry points (csrc/ln_act.hip), for a sanitizer build of the host code on a
// machine without a GPU: every call below is refused, or has nothing to do, before any launch.
//
//   cd warpconvnet_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       ln_act.hip adaln.hip ../../tools/row_permute_host_check.cpp -I../../include -o /tmp/row_permute_host_check \
//     && /tmp/row_permute_host_check
#include <cstdint>
#include <cstdio>
#include <limits>

#include "wcn.h"

static int failures = 0;
#define EXPECT(call, want)                                                        \
  do {                                                                            \
    const int got = (call);                                                       \
    if (got != (want)) {                                                          \
      std::printf("line %d: %s = %d, expected %d\n", __LINE__, #call, got, want); \
      ++failures;                                                                 \
    }                                                                             \
  } while (0)

int main() {
  alignas(16) static float rows_buf[5 * 64];
  alignas(16) static float vec[64];
  alignas(16) static float stats[5 * 2];
  alignas(16) static int64_t index[5] = {4, 3, 2, 1, 0};
  alignas(16) static unsigned char workspace[2 * 64 * sizeof(float)];
  void* x = rows_buf;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const int f32 = WCN_F32;

  // zero rows: success, whatever the pointers are
  EXPECT(wcn_ln_permute_fwd(nullptr, nullptr, nullptr, nullptr, 0, 64, 1e-5f, f32, nullptr, nullptr, nullptr), WCN_SUCCESS);
  EXPECT(wcn_ln_permute_bwd(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 64, f32, nullptr, nullptr, nullptr, nullptr, 0, nullptr),
         WCN_SUCCESS);
  EXPECT(wcn_permute_add(nullptr, nullptr, nullptr, nullptr, 0, 0, 64, f32, nullptr, nullptr), WCN_SUCCESS);
  // widths and dtypes outside the domain
  const int bad_widths[] = {12, 4, 0, 2056, -8};
  for (int c : bad_widths) {
    EXPECT(wcn_ln_permute_fwd(x, index, nullptr, nullptr, 5, c, 1e-5f, f32, x, stats, nullptr), WCN_ERROR_UNSUPPORTED_CONFIG);
    EXPECT(wcn_ln_permute_bwd(x, x, index, nullptr, stats, 5, c, f32, x, nullptr, nullptr, nullptr, 0, nullptr),
           WCN_ERROR_UNSUPPORTED_CONFIG);
    EXPECT(wcn_permute_add(x, index, x, nullptr, 0, 5, c, f32, x, nullptr), WCN_ERROR_UNSUPPORTED_CONFIG);
  }
  EXPECT(wcn_ln_permute_fwd(x, index, nullptr, nullptr, 5, 64, 1e-5f, 3, x, stats, nullptr), WCN_ERROR_UNSUPPORTED_CONFIG);
  EXPECT(wcn_permute_add(x, index, x, nullptr, 0, 5, 64, -1, x, nullptr), WCN_ERROR_UNSUPPORTED_CONFIG);
  // row counts
  const int64_t bad_rows[] = {-1, (int64_t)1 << 31};
  for (int64_t r : bad_rows) {
    EXPECT(wcn_ln_permute_fwd(x, index, nullptr, nullptr, r, 64, 1e-5f, f32, x, stats, nullptr), WCN_ERROR_INVALID_PARAMETERS);
    EXPECT(wcn_ln_permute_bwd(x, x, index, nullptr, stats, r, 64, f32, x, nullptr, nullptr, nullptr, 0, nullptr),
           WCN_ERROR_INVALID_PARAMETERS);
    EXPECT(wcn_permute_add(x, index, x, nullptr, 0, r, 64, f32, x, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  }
  // null and misaligned pointers, half an affine pair, eps, workspace, the scale switch
  EXPECT(wcn_ln_permute_fwd(nullptr, index, nullptr, nullptr, 5, 64, 1e-5f, f32, x, stats, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_fwd(x, nullptr, nullptr, nullptr, 5, 64, 1e-5f, f32, x, stats, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_fwd(x, index, nullptr, nullptr, 5, 64, 1e-5f, f32, nullptr, stats, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_fwd(x, index, nullptr, nullptr, 5, 64, 1e-5f, f32, x, nullptr, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_fwd(x, index, vec, nullptr, 5, 64, 1e-5f, f32, x, stats, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_fwd(x, index, nullptr, vec, 5, 64, 1e-5f, f32, x, stats, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_fwd(x, index, nullptr, nullptr, 5, 64, nan, f32, x, stats, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_fwd(x, index, nullptr, nullptr, 5, 64, -1.f, f32, x, stats, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_fwd(rows_buf + 1, index, nullptr, nullptr, 5, 64, 1e-5f, f32, x, stats, nullptr),
         WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_bwd(nullptr, x, index, nullptr, stats, 5, 64, f32, x, nullptr, nullptr, nullptr, 0, nullptr),
         WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_bwd(x, x, nullptr, nullptr, stats, 5, 64, f32, x, nullptr, nullptr, nullptr, 0, nullptr),
         WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_bwd(x, x, index, nullptr, nullptr, 5, 64, f32, x, nullptr, nullptr, nullptr, 0, nullptr),
         WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_bwd(x, x, index, vec, stats, 5, 64, f32, x, vec, vec, workspace, sizeof(workspace) - 1, nullptr),
         WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_bwd(x, x, index, vec, stats, 5, 64, f32, x, nullptr, vec, workspace, sizeof(workspace), nullptr),
         WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_ln_permute_bwd(x, x, index, vec, stats, 5, 64, f32, x, vec, vec, nullptr, sizeof(workspace), nullptr),
         WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_permute_add(nullptr, index, x, nullptr, 0, 5, 64, f32, x, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_permute_add(x, nullptr, x, nullptr, 0, 5, 64, f32, x, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_permute_add(x, index, x, nullptr, 0, 5, 64, f32, nullptr, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_permute_add(x, index, x, vec, 2, 5, 64, f32, x, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT(wcn_permute_add(x, index, rows_buf + 1, nullptr, 0, 5, 64, f32, x, nullptr), WCN_ERROR_INVALID_PARAMETERS);
  EXPECT((int)wcn_ln_act_workspace_bytes(5, 64), (int)sizeof(workspace));

  std::printf(failures ? "%d check(s) failed\n" : "all argument checks passed (%d failures)\n", failures);
  return failures ? 1 : 0;
}
