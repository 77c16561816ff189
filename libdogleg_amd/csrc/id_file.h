// id_file.h -- the id file of the multi-GPU environment contract (id_file.cpp; not installed).  Plain C++: no HIP
// header, no backend header -- tests/c/id_file_main.cpp links id_file.cpp alone.
#pragma once

// include/dogleg.h declares the same two
extern "C" int dogleg_amd_id_file_publish(const char* path, const void* id128, const char* run_id);
extern "C" int dogleg_amd_id_file_wait(const char* path, void* id128_out, const char* run_id, int timeout_ms);

// the launch's run id: DOGLEG_AMD_RUN_ID, else TORCHELASTIC_RUN_ID, else empty
__attribute__((visibility("hidden"))) const char* env_run_id();
