// driver_msg.h -- how the host driver's files report on stderr (not installed; needs <cstdio> only)
#pragma once
#include <cstdio>

#define MSG(...) do { fprintf(stderr, "libdogleg_amd: " __VA_ARGS__); fputc('\n', stderr); } while(0)
