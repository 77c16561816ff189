// sparse_region.h -- host-only planner of the sparse factorisation's launches (K5).  Plain C++
// on the symbolic phase's SymHost, no HIP: sparse_factor.hip uploads what comes out of here, dlg_sparse_region_probe
// and tests/c/region_plan_main.cpp run it on the CPU.  Errors go through (char* err, size_t len), as in sym_analyze.
#pragma once
#include "sparse_symbolic.h"
#include <cstddef>

// what steers the one-launch regions, read from the environment and the device in one place (region_knobs_env)
struct RegionKnobs
{
  int ncu, cap, rmax;      // CUs; supernodes a region may hold (DOGLEG_AMD_PERSIST_MAX); replicas of a supernode, 1 .. 8 (DOGLEG_AMD_FRONT_REPLICAS)
  bool slices, persist;    // not DOGLEG_AMD_NO_FRONT_SLICES (replicas may keep a slice of the update matrix), not DOGLEG_AMD_NO_PERSIST
  bool lower, timing;      // not DOGLEG_AMD_NO_LOWER_REGION (a partition's region below the cut); DOGLEG_AMD_TIMING (a line per region on stderr)
};
RegionKnobs region_knobs_env(int ncu);

// per-level launch parameters of the factor and update kernels, [nlevels] each; nt, lds, leaf, stage: k_factor_level's
// block size, dynamic LDS, lean instantiation, update matrices of childless supernodes staged.  Its own knobs
// (DOGLEG_AMD_NO_LEAF_KERNEL, _MF_NT, _NO_UPDATE_MFMA, _NO_SYRK_FUSE, _SYM_DEBUG) are read where they apply.
struct FacLevels { std::vector<int> nt, lds, leaf, stage, upd_coop, upd_lds, upd_nw, syrk_lds, syrk_nt, syrk_kc, syrk_fused, fin_ny; };
int fac_level_params(const SymHost& H, FacLevels& L, char* err, size_t len);

// the schedule of one one-launch region: levels level0 .. level1 (level0 == H.nlevels: none)
struct RegionPlan
{
  int level0 = 0, level1 = -1, lds = 0, stage = 0, nwg = 0;
  bool acc_any = false;                 // an update matrix of the region is summed in HBM: the shadow scratch is needed
  std::vector<FwItem> item;             // work items (supernode x replica), in launch order
  std::vector<MfChild> rec;             // the region's copy of the children records, behind it those of the replicas
  std::vector<uint16_t> dst;            // ... and of the destination lists
};
// levels [lo_min, hi], as far down from hi as the conditions hold
RegionPlan region_plan(const SymHost& H, const FacLevels& L, int lo_min, int hi, const RegionKnobs& K);
// 0, or nonzero with the violated invariant in err; stats (may be null): {sliced workgroups, supernodes whose update matrix stays in HBM}
int region_check(const SymHost& H, const RegionPlan& R, long* stats, char* err, size_t len);
// 64-bit FNV-1a over the fields (not the bytes) of a plan / of the level parameters
uint64_t region_plan_hash(const RegionPlan& R);
uint64_t fac_levels_hash(const FacLevels& L);
