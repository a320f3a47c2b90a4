// Library-wide pieces of the C ABI: version and thread-local error string.  This is also the translation unit of the host-only
// API sources (included at the end), so that the list of units -- which the test-suite's CPU build repeats -- names kernels' files
// and this one, whatever host code is split off them.
#include "p2p_common.h"

namespace p2p {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace p2p

#ifdef P2P_EXPERIMENT
extern "C" int p2p_version(void) { return 112 | P2P_VERSION_EXPERIMENT; }
#else
extern "C" int p2p_version(void) { return 112; }
#endif
extern "C" const char *p2p_last_error(void) { return p2p::g_err; }

#include "coarse_api.hip"        // coarse stage: handle, workspace, entry points
#include "operators_api.hip"     // the matching operators on their own: argument checks, entry points
#include "regress_api.hip"       // fine stage: handle, modes, entry points
#include "preprocess.hip"       // bicubic resize + normalisation (kernels and their entry points; no unit of its own)
