// driver_cache.hip -- what outlives a solve (the reference allocates and frees everything per solve,
// dogleg.c:1479-1562, 1694-1750; there a solve takes seconds -- here the set-up WAS the solve: 90 of the 100 ms of a
// 5-trial device-callback solve of config #4).  Between dogleg_optimize* calls the library keeps
//   * ONE idle backend (device buffers, streams, the uploaded pattern and schedules, hipFuncSetAttribute'd
//     kernels): the next solve of the same shape takes it over (dlg_backend_reset); a sparse solve whose
//     pattern is the one it was set up for skips the symbolic phase and every upload;
//   * the page-locked host buffers of the operating points (hipHostMalloc of 2 x 190 MB costs tens of ms).
// DOGLEG_AMD_NO_BACKEND_CACHE=1 turns both off; dogleg_amd_release_cache() frees them.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>
#include "driver_internal.h"
#include "dense_batch.h"

namespace {

struct ParkedBackend { dlg_backend_t* be = nullptr; int type = 0, N = 0, M = 0, nnz = 0, flags = 0, device = 0; unsigned long long env = 0; };
// (a backend reads its DOGLEG_AMD_* knobs when it is created: one made under other knobs is not taken over)
extern "C" char** environ;
unsigned long long env_knobs_hash()
{
  unsigned long long h = 1469598103934665603ull;
  for(char** e = environ; e && *e; e++)
    if(!strncmp(*e, "DOGLEG_AMD_", 11) || !strncmp(*e, "DLG_", 4))
    {
      unsigned long long g = 1469598103934665603ull;
      for(const char* c = *e; *c; c++) { g ^= (unsigned char)*c; g *= 1099511628211ull; }
      h += g;                               // order-independent
    }
  return h;
}
struct PinnedBuf { void* p; size_t bytes; };
std::mutex g_cache_mu;
ParkedBackend g_parked;
std::vector<PinnedBuf> g_pinned_pool;
size_t g_pinned_pool_bytes = 0;
constexpr size_t PINNED_POOL_CAP = (size_t)4 << 30;

} // namespace

bool cache_on() { static const bool on = getenv("DOGLEG_AMD_NO_BACKEND_CACHE") == nullptr; return on; }

dlg_backend_t* take_parked(int type, int N, int M, int nnz, int flags, int device)
{
  // (device -1 = the calling thread's current GPU, as dlg_backend_create resolves it: a backend parked on
  // another GPU is not this solve's -- a device callback would get pointers and a stream of the wrong device)
  if(device < 0 && hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  std::lock_guard<std::mutex> lk(g_cache_mu);
  ParkedBackend& P = g_parked;
  if(!P.be || P.type != type || P.N != N || P.M != M || P.nnz != nnz || P.flags != flags || P.device != device ||
     P.env != env_knobs_hash()) return nullptr;
  dlg_backend_t* be = P.be;
  P.be = nullptr;
  return be;
}
void park_backend(dlg_backend_t* be, int type, int N, int M, int nnz, int flags)
{
  if(!be) return;
  dlg_backend_t* old = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    old = g_parked.be;
    g_parked.be = be; g_parked.type = type; g_parked.N = N; g_parked.M = M; g_parked.nnz = nnz; g_parked.flags = flags;
    g_parked.device = dlg_backend_device(be); g_parked.env = env_knobs_hash();
  }
  if(old) dlg_backend_destroy(old);
}
void* pinned_take(size_t bytes)
{
  std::lock_guard<std::mutex> lk(g_cache_mu);
  for(size_t i = 0; i < g_pinned_pool.size(); i++)
    if(g_pinned_pool[i].bytes == bytes)
    {
      void* p = g_pinned_pool[i].p;
      g_pinned_pool_bytes -= bytes;
      g_pinned_pool[i] = g_pinned_pool.back(); g_pinned_pool.pop_back();
      return p;
    }
  return nullptr;
}
void pinned_give(void* p, size_t bytes)
{
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    if(cache_on() && g_pinned_pool_bytes + bytes <= PINNED_POOL_CAP && g_pinned_pool.size() < 64)
    { g_pinned_pool.push_back({p, bytes}); g_pinned_pool_bytes += bytes; return; }
  }
  (void)hipHostFree(p);
}

// what the library keeps between solves (the idle backend with its device memory, page-locked host buffers)
extern "C" void dogleg_amd_release_cache(void)
{
  dlg_backend_t* be = nullptr;
  std::vector<PinnedBuf> pool;
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    be = g_parked.be; g_parked.be = nullptr;
    pool.swap(g_pinned_pool); g_pinned_pool_bytes = 0;
  }
  if(be) dlg_backend_destroy(be);
  for(const PinnedBuf& b : pool) (void)hipHostFree(b.p);
  dlg_dense_batch_release();
  robust_release_cache();
  bounds_release_cache();
}
