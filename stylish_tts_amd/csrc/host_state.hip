// Process-wide host state of libstylish_hip.so: the error string behind sty_last_error, the single-stream and
// deterministic switches, and the in-situ profiler behind ProfScope, with the entries that set and read them.
#include <cxxabi.h>
#include <stdarg.h>
#include <stdlib.h>

#include <map>
#include <string>

#include "run.h"

namespace sty {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int hip_fail(hipError_t e, const char* what) {
  set_error("HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
  return STY_EHIP;
}

// ---------------------------------------------------------------------------------------------------
// in-situ kernel timing
// ---------------------------------------------------------------------------------------------------
struct ProfEntry {
  std::string family;
  double flops, bytes;
  hipEvent_t a, b;
  const void* fn = nullptr;  // host-side handle of the kernel launched inside the scope (the last one, if several)
};
thread_local const void* g_last_kernel = nullptr;
static bool g_single_stream = false;  // sty_set_single_stream
bool single_stream_mode() { return g_single_stream; }
static bool g_deterministic = false;  // sty_set_deterministic
bool deterministic_mode() { return g_deterministic; }
static bool g_prof_on = false;
static std::string g_prof_only;  // non-empty: only launches of this family are timed (sty_prof_only)
static std::vector<ProfEntry> g_prof;
static std::vector<hipEvent_t> g_evpool;
static hipEvent_t prof_event() {
  if (!g_evpool.empty()) {
    hipEvent_t e = g_evpool.back();
    g_evpool.pop_back();
    return e;
  }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}
// STY_PROF_SHAPES=1: one row per (kernel family, problem shape) instead of one per family
static const bool g_prof_shapes = getenv("STY_PROF_SHAPES") != nullptr;
ProfScope::ProfScope(const char* family, double flops, double bytes, hipStream_t s, const char* detail) : st(s) {
  if (!g_prof_on) return;
  if (!g_prof_only.empty() && g_prof_only != family) return;
  std::string name(family);
  if (g_prof_shapes && detail) name = name + " " + detail;
  ProfEntry e{name, flops, bytes, prof_event(), prof_event()};
  if (!e.a || !e.b) return;
  (void)hipEventRecord(e.a, st);
  slot = (int)g_prof.size();
  g_prof.push_back(e);
}
ProfScope::~ProfScope() {
  if (slot >= 0) {
    (void)hipEventRecord(g_prof[slot].b, st);
    g_prof[slot].fn = g_last_kernel;
  }
}
// "void sty::convp16_kernel<2, 0, 0, true, true>(sty::ConvArgs, int, int, int, int)" -> "convp16_kernel<2, 0, 0, true, true>":
// the kernel's name as rocprofv3 --kernel-trace prints it, minus return type, namespaces and the argument list
static std::string kernel_inst_name(const void* fn, hipStream_t st) {
  static std::map<const void*, std::string> cache;
  if (!fn) return "";
  auto it = cache.find(fn);
  if (it != cache.end()) return it->second;
  std::string out;
  const char* mangled = hipKernelNameRefByPtr(fn, st);
  if (mangled) {
    int status = 0;
    char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
    std::string d = (status == 0 && dem) ? dem : mangled;
    free(dem);
    int depth = 0;  // cut the argument list: the first '(' outside template brackets ("(anonymous namespace)" starts inside "sty::")
    size_t cut = d.size();
    for (size_t i = 0; i < d.size(); ++i) {
      if (d[i] == '<') ++depth;
      if (d[i] == '>') --depth;
      if (d[i] == '(' && depth == 0 && d.compare(i, 21, "(anonymous namespace)") != 0) {
        cut = i;
        break;
      }
    }
    d = d.substr(0, cut);
    if (d.compare(0, 5, "void ") == 0) d = d.substr(5);
    for (const char* ns : {"sty::(anonymous namespace)::", "sty::"})
      if (d.compare(0, strlen(ns), ns) == 0) d = d.substr(strlen(ns));
    out = d;
  }
  cache[fn] = out;
  return out;
}

}  // namespace sty

using namespace sty;

extern "C" {

int sty_prof_enable(int on) {
  g_prof_on = on != 0;
  return STY_OK;
}
int sty_set_single_stream(int on) {
  sty::g_single_stream = on != 0;
  return STY_OK;
}
int sty_set_deterministic(int on) {
  sty::g_deterministic = on != 0;
  return STY_OK;
}
int sty_get_deterministic(void) { return sty::g_deterministic ? 1 : 0; }
int sty_prof_only(const char* family) {
  g_prof_only = family ? family : "";
  return STY_OK;
}
int sty_prof_report(sty_prof_row* rows, int cap) {
  STY_HIP(hipDeviceSynchronize());
  // one row per (family, instantiation): the family is the launch site's label (tile parameter + bf16 marker), the instantiation
  // the kernel's own name as the tracer prints it
  std::vector<sty_prof_row> agg;
  for (ProfEntry& e : g_prof) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) ms = 0.f;
    g_evpool.push_back(e.a);
    g_evpool.push_back(e.b);
    const std::string inst = kernel_inst_name(e.fn, nullptr);
    sty_prof_row* r = nullptr;
    for (auto& x : agg)
      if (!strncmp(x.name, e.family.c_str(), sizeof(x.name) - 1) && !strncmp(x.inst, inst.c_str(), sizeof(x.inst) - 1)) r = &x;
    if (!r) {
      sty_prof_row n;
      memset(&n, 0, sizeof(n));
      strncpy(n.name, e.family.c_str(), sizeof(n.name) - 1);
      strncpy(n.inst, inst.c_str(), sizeof(n.inst) - 1);
      agg.push_back(n);
      r = &agg.back();
    }
    r->launches += 1;
    r->ms += ms;
    r->flops += e.flops;
    r->bytes += e.bytes;
  }
  g_prof.clear();
  for (int i = 0; i < (int)agg.size() && i < cap && rows; ++i) rows[i] = agg[i];
  return (int)agg.size();
}

int sty_version(void) { return 1; }
const char* sty_last_error(void) { return g_err; }

}  // extern "C"
