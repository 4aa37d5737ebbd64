// Library identification and the read-only process configuration (no device work).
#include <stdlib.h>

#include "sea_common.h"

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
