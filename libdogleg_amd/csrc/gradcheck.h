// gradcheck.h -- the Jacobian check of gradcheck.hip as the driver sees it (not installed).  The arguments are checked
// by the caller (api_extensions.cpp: dogleg_amd_check_jacobian_device*); 0 or more / -1 with a message on stderr.
#pragma once
#include "../../include/dogleg.h"

// sparse (nnz > 0, the pattern checked) or dense (nnz == 0): returns the records written to bad
int  dlg_gradcheck_run(const double* p0, unsigned int N, unsigned int M, unsigned int nnz, const int* colptr,
                       const int* rowidx, dogleg_callback_device_t* f, void* cookie, double delta, double rtol, double atol,
                       int flags, dogleg_amd_jacobian_report_t* report, double* var_error,
                       dogleg_amd_jacobian_entry_t* bad, int max_bad);
int  dlg_gradcheck_batch_run(const double* p0, unsigned int B, unsigned int N, unsigned int M,
                             dogleg_callback_device_batch_t* f, void* cookie, double delta, double rtol, double atol,
                             dogleg_amd_jacobian_report_t* reports, dogleg_amd_jacobian_entry_t* bad, int max_bad,
                             long long* nbad_total);
// reported / observed of variable var per measurement, [M][2], for dogleg_amd_testGradient_device
int  dlg_gradcheck_table(unsigned int var, const double* p0, unsigned int N, unsigned int M, unsigned int nnz,
                         const int* colptr, const int* rowidx, dogleg_callback_device_t* f, void* cookie, double delta,
                         double* table);
int  dlg_gradcheck_last_stats(double* out, int n);
