// Library identification, the read-only process configuration and the host-only report of the M2 plan (no device work).
#include <stdlib.h>

#include "sea_common.h"
#include "upsample_plan.h"

#ifndef SEA_BUILD_STAMP
#define SEA_BUILD_STAMP "unknown"
#endif

extern "C" int sea_abi_version(void) { return 3; }
extern "C" const char* sea_build_info(void) { return "libsea_hip gfx950 " SEA_BUILD_STAMP; }

namespace sea {

// The one place under csrc/ that reads the environment: initialised once (thread-safe), immutable afterwards.
const ProcessConfig& process_config() {
  static const ProcessConfig cfg = [] {
    ProcessConfig c;
    const char* x = getenv("SEA_XCD_ORDER");
    c.xcd_order = (x && x[0] >= '0' && x[0] <= '2') ? x[0] - '0' : 1;
    const char* g = getenv("SEA_UPSAMPLE_GENERAL");
    c.upsample_general = (g && g[0] == '1') ? 1 : 0;
    return c;
  }();
  return cfg;
}

}  // namespace sea

extern "C" int sea_process_config(int which) {
  const sea::ProcessConfig& c = sea::process_config();
  return which == SEA_CONFIG_XCD_ORDER ? c.xcd_order : (which == SEA_CONFIG_UPSAMPLE_GENERAL ? c.upsample_general : -1);
}

// host only: the plan of an M2 / tap-gather call (upsample_plan.h), without the call
extern "C" int sea_upsample_plan(int op, int64_t planes_or_batch, int C, int h, int w, int H, int W, int64_t pixel_stride,
                                 size_t src_addr, size_t dst_addr, int general_only, int xcd_order, int32_t out[20]) {
  SEA_CHECK_ARG(out != nullptr);
  sea::UpsamplePlan p;
  const int rc = sea::upsample_plan(sea::UpsampleQuery{op, planes_or_batch, C, h, w, H, W, pixel_stride, src_addr, dst_addr,
                                                       general_only != 0, xcd_order}, &p);
  const int v[20] = {p.kernel, p.S, p.grid_x, p.grid_y, p.threads, (int)p.lds, p.chunk, p.nchunks, (int)(uint32_t)p.total,
                     (int)(p.total >> 32), p.xo, p.nt, p.lcols, p.RP, p.bands, p.per_xcd, p.TI, p.RMAX, p.nbh, p.nbw};
  for (int i = 0; i < 20; ++i) out[i] = v[i];
  return rc;
}
