// ABI bookkeeping entry points of libseld_hip.so.
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include "common.h"
#include "env.h"

namespace seld {
thread_local int g_last_hip_error = 0;

static SeldEnv g_env;
static bool g_env_loaded = false;
static std::mutex g_env_mutex;

static bool flag(const char* name) { const char* e = getenv(name); return e && *e; }

static void load_env_locked() {
    SeldEnv e;
    if (const char* c = getenv("SELD_CONV_CFG")) {
        int a = 0, b = 0;
        if (sscanf(c, "%d,%d", &a, &b) == 2 && a >= 1 && a <= 12 && b >= 1 && b <= 4) { e.conv_cfg_ct = a; e.conv_cfg_pt = b; }
    }
    e.conv_no_smallk = flag("SELD_CONV_NO_SMALLK");
    e.conv_no_hcq = flag("SELD_CONV_NO_HCQ");
    e.deterministic = flag("SELD_DETERMINISTIC");
    e.mha_no_mfma = flag("SELD_MHA_NO_MFMA");
    g_env = e;
    g_env_loaded = true;
}

const SeldEnv& env() {
    if (!g_env_loaded) {
        std::lock_guard<std::mutex> lk(g_env_mutex);
        if (!g_env_loaded) load_env_locked();
    }
    return g_env;
}
}  // namespace seld

/* Re-read the SELD_* environment switches (they are read once, at first use).  Not thread safe against
 * concurrent launches: call it between launches (the tests do, after changing the environment). */
extern "C" int seld_env_reload(void) {
    std::lock_guard<std::mutex> lk(seld::g_env_mutex);
    seld::load_env_locked();
    return SELD_OK;
}

extern "C" int seld_abi_version(void) { return 2; }
extern "C" const char* seld_build_arch(void) { return "gfx950"; }
extern "C" int seld_last_hip_error(void) { return seld::g_last_hip_error; }
