// id_file_main.cpp -- the id-file rendezvous as a stand-alone program, so that it can be built with
// -fsanitize=address,undefined (tests/test_library_cpu.py).  Links id_file.cpp only: no HIP, no backend.
//   id_file_main DIR
// runs every case in DIR (which must exist and be empty); prints "ok" and exits 0, or names the case that failed.
#include <cstdio>
#include <cstring>
#include <string>
#include "id_file.h"

static bool write_bytes(const std::string& path, const unsigned char* b, size_t n)
{
  FILE* f = fopen(path.c_str(), "wb");
  if(!f) return false;
  const bool ok = fwrite(b, 1, n, f) == n;
  return fclose(f) == 0 && ok;
}
static size_t read_bytes(const std::string& path, unsigned char* b, size_t cap)
{
  FILE* f = fopen(path.c_str(), "rb");
  if(!f) return 0;
  const size_t n = fread(b, 1, cap, f);
  fclose(f);
  return n;
}
#define CHECK(c) do { if(!(c)) { printf("failed: %s (line %d)\n", #c, __LINE__); return 1; } } while(0)

int main(int argc, char** argv)
{
  if(argc != 2) { fprintf(stderr, "usage: id_file_main DIR\n"); return 2; }
  const std::string dir = argv[1];
  unsigned char id[128], got[128];
  for(int i = 0; i < 128; i++) id[i] = (unsigned char)(37*i + 11);

  // publish, then wait: the id comes back, under the run id it was written for and under none
  const std::string a = dir + "/a.id";
  CHECK(dogleg_amd_id_file_publish(a.c_str(), id, "launch-1") == 0);
  memset(got, 0, sizeof(got));
  CHECK(dogleg_amd_id_file_wait(a.c_str(), got, "launch-1", 1000) == 0 && !memcmp(got, id, 128));
  const std::string n = dir + "/none.id";
  CHECK(dogleg_amd_id_file_publish(n.c_str(), id, nullptr) == 0);
  memset(got, 0, sizeof(got));
  CHECK(dogleg_amd_id_file_wait(n.c_str(), got, "", 1000) == 0 && !memcmp(got, id, 128));
  unsigned char rec[256];
  CHECK(read_bytes(a, rec, sizeof(rec)) == 144 && !memcmp(rec, id, 128) && !memcmp(rec + 128, "DLGAMD01", 8));
  CHECK(read_bytes(a + ".tmp", rec, sizeof(rec)) == 0);              // (tmp + rename: nothing is left behind)

  // a file written under another run id: not this launch's, the wait runs out and writes nothing
  memset(got, 0xee, sizeof(got));
  CHECK(dogleg_amd_id_file_wait(a.c_str(), got, "launch-2", 60) == -1);
  for(int i = 0; i < 128; i++) CHECK(got[i] == 0xee);
  // no file at all, and bad arguments
  CHECK(dogleg_amd_id_file_wait((dir + "/missing.id").c_str(), got, "launch-1", 40) == -1);
  CHECK(dogleg_amd_id_file_wait(nullptr, got, "", 10) == -1 && dogleg_amd_id_file_wait(a.c_str(), nullptr, "", 10) == -1);
  CHECK(dogleg_amd_id_file_publish(nullptr, id, "") == -1 && dogleg_amd_id_file_publish(a.c_str(), nullptr, "") == -1);
  CHECK(dogleg_amd_id_file_publish((dir + "/no/such/dir.id").c_str(), id, "") == -1);

  // a truncated file and one that is one byte too long: both are some other file, whatever their first bytes say
  CHECK(read_bytes(a, rec, sizeof(rec)) == 144);
  const std::string t = dir + "/short.id", l = dir + "/long.id";
  CHECK(write_bytes(t, rec, 143));
  CHECK(dogleg_amd_id_file_wait(t.c_str(), got, "launch-1", 60) == -1);
  rec[144] = 0;
  CHECK(write_bytes(l, rec, 145));
  CHECK(dogleg_amd_id_file_wait(l.c_str(), got, "launch-1", 60) == -1);
  CHECK(write_bytes(t, rec, 0));
  CHECK(dogleg_amd_id_file_wait(t.c_str(), got, "launch-1", 40) == -1);
  for(int i = 0; i < 128; i++) CHECK(got[i] == 0xee);
  // and the whole record again: taken
  CHECK(write_bytes(t, rec, 144));
  CHECK(dogleg_amd_id_file_wait(t.c_str(), got, "launch-1", 1000) == 0 && !memcmp(got, id, 128));
  printf("ok\n");
  return 0;
}
