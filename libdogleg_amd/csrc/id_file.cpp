// id_file.cpp -- the id file of the environment contract (driver_comm.hip: env_communicator).  144 bytes: the
// 128-byte RCCL id, the tag "DLGAMD01", and the 64-bit FNV-1a hash of the launch's run id (DOGLEG_AMD_RUN_ID, else
// TORCHELASTIC_RUN_ID, else empty).  A reader takes only a complete file whose run id is its own: a file an earlier
// launch left at the path under another run id is skipped (under the SAME run id -- or none -- the path has to be
// fresh for each launch; rank 0 removes what it finds before it makes the id, which narrows that window, it cannot
// close it).  Written as tmp + rename: never seen half.
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <string>
#include <time.h>
#include "driver_msg.h"
#include "id_file.h"

namespace {
unsigned long long run_id_hash(const char* run_id)
{
  unsigned long long g = 1469598103934665603ull;
  for(const char* c = run_id ? run_id : ""; *c; c++) { g ^= (unsigned char)*c; g *= 1099511628211ull; }
  return g;
}
constexpr size_t ID_FILE_BYTES = 144;
} // namespace

const char* env_run_id()
{
  const char* r = getenv("DOGLEG_AMD_RUN_ID");
  if(!r) r = getenv("TORCHELASTIC_RUN_ID");
  return r ? r : "";
}

extern "C" int dogleg_amd_id_file_publish(const char* path, const void* id128, const char* run_id)
{
  if(!path || !id128) { MSG("dogleg_amd_id_file_publish: bad arguments"); return -1; }
  unsigned char rec[ID_FILE_BYTES];
  memcpy(rec, id128, 128); memcpy(rec + 128, "DLGAMD01", 8);
  const unsigned long long h = run_id_hash(run_id);
  memcpy(rec + 136, &h, 8);
  const std::string tmp = std::string(path) + ".tmp";
  FILE* f = fopen(tmp.c_str(), "wb");
  if(!f || fwrite(rec, 1, ID_FILE_BYTES, f) != ID_FILE_BYTES) { MSG("cannot write %s", tmp.c_str()); if(f) fclose(f); return -1; }
  if(fclose(f) != 0) { MSG("cannot write %s", tmp.c_str()); return -1; }
  if(rename(tmp.c_str(), path) != 0) { MSG("cannot rename %s to %s", tmp.c_str(), path); return -1; }
  return 0;
}
extern "C" int dogleg_amd_id_file_wait(const char* path, void* id128_out, const char* run_id, int timeout_ms)
{
  if(!path || !id128_out) { MSG("dogleg_amd_id_file_wait: bad arguments"); return -1; }
  const unsigned long long want = run_id_hash(run_id);
  const auto t0 = std::chrono::steady_clock::now();
  for(;;)
  {
    unsigned char rec[ID_FILE_BYTES + 1];
    FILE* f = fopen(path, "rb");
    if(f)
    {
      const size_t n = fread(rec, 1, sizeof(rec), f);
      fclose(f);
      unsigned long long h = 0;
      if(n == ID_FILE_BYTES) memcpy(&h, rec + 136, 8);
      if(n == ID_FILE_BYTES && !memcmp(rec + 128, "DLGAMD01", 8) && h == want) { memcpy(id128_out, rec, 128); return 0; }
    }
    if(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() >= (double)timeout_ms) break;
    struct timespec ts = {0, 20000000}; nanosleep(&ts, nullptr);
  }
  MSG("no RCCL id of this launch in %s after %d ms", path, timeout_ms);
  return -1;
}
