// driver_comm.cpp -- multi-GPU behind dogleg.h (extension, not in the reference; see include/dogleg.h): which
// communicator a solve uses, and how its backend becomes one rank of it.  No HIP call: everything goes through
// dlg_backend.h.
#include <cstdlib>
#include <cstring>
#include <mutex>
#include "driver_internal.h"
#include "id_file.h"

namespace {

thread_local Comm t_comm;
// the environment contract: the RCCL communicator is made once per process and adopted by every solve
struct EnvComm { bool tried = false, ok = false; int rank = 0, nranks = 1, device = -1; dlg_backend_t* holder = nullptr; };
EnvComm g_env_comm;

// DOGLEG_AMD_WORLD_SIZE (> 1), DOGLEG_AMD_RANK, DOGLEG_AMD_LOCAL_RANK (the GPU; default: the rank),
// DOGLEG_AMD_RCCL_ID_FILE: rank 0 writes the RCCL id there (dogleg_amd_id_file_publish), the others wait for it
// (dogleg_amd_id_file_wait, two minutes; DOGLEG_AMD_RUN_ID names the launch).  The communicator is made once per
// process -- a backend that only holds it -- and shared by every solve; solves may start on several threads.
std::mutex g_env_comm_mu;
bool env_world() { const char* ws = getenv("DOGLEG_AMD_WORLD_SIZE"); return ws && atoi(ws) > 1; }
bool env_communicator(Comm* cm)
{
  std::lock_guard<std::mutex> lk(g_env_comm_mu);
  EnvComm& E = g_env_comm;
  if(!E.tried)
  {
    E.tried = true;
    const char* ws = getenv("DOGLEG_AMD_WORLD_SIZE");
    const int n = ws ? atoi(ws) : 1;
    if(n > 1 || (ws && getenv("DOGLEG_AMD_FORCE_COMM")))
    {
      const char* rk = getenv("DOGLEG_AMD_RANK"); const char* lr = getenv("DOGLEG_AMD_LOCAL_RANK");
      const char* idf = getenv("DOGLEG_AMD_RCCL_ID_FILE");
      if(!rk || !idf) { MSG("DOGLEG_AMD_WORLD_SIZE=%d needs DOGLEG_AMD_RANK and DOGLEG_AMD_RCCL_ID_FILE", n); return false; }
      E.rank = atoi(rk); E.nranks = n; E.device = lr ? atoi(lr) : E.rank;
      if(E.rank < 0 || E.rank >= n) { MSG("DOGLEG_AMD_RANK=%d of %d", E.rank, n); return false; }
      unsigned char id[128];
      if(E.rank == 0)
      {
        (void)remove(idf);                          // (what an earlier launch left there)
        if(dlg_rccl_unique_id(id) != DLG_OK) { MSG("RCCL id: %s", dlg_last_error()); return false; }
        if(dogleg_amd_id_file_publish(idf, id, env_run_id()) != 0) return false;
      }
      else if(dogleg_amd_id_file_wait(idf, id, env_run_id(), 120000) != 0) return false;
      // (a backend with nothing in it but the communicator: dlg_backend_share_rccl hands it to the solves)
      if(dlg_backend_create(&E.holder, DLG_DENSE_PRODUCTS, 1, 0, 0, 0, E.device) != DLG_OK ||
         dlg_backend_init_rccl(E.holder, E.rank, E.nranks, id) != DLG_OK)
      { MSG("cannot make the process's RCCL communicator: %s", dlg_last_error()); return false; }
      E.ok = true;
    }
  }
  if(E.tried && !E.ok && env_world()) return false;
  if(E.ok) { cm->rank = E.rank; cm->nranks = E.nranks; cm->device = E.device; cm->set = true; }
  return true;
}

} // namespace

bool solve_communicator(Comm* cm)
{
  *cm = t_comm;
  return cm->set || env_communicator(cm);
}

bool attach_communicator(Driver* d, const Comm& cm)
{
  const dogleg_solverContext_t* ctx = &d->pub;
  d->rank = cm.rank; d->nranks = cm.nranks; d->row0 = 0; d->row1 = ctx->Nmeasurements;
  // Measurement rows are the sharded unit (dogleg.c:253-260, 269-278, 712-714).  Sparse: the subtree
  // partition of the elimination tree; dense: contiguous rows, JtJ summed.  (dense-products: the
  // callback has already summed over the rows -- every rank does the same work: replicas.)
  if(!cm.set || ctx->solve_type == DOGLEG_DENSE_PRODUCTS) return true;
  if(ctx->solve_type == DOGLEG_SPARSE)
  { if(!be_ok(dlg_backend_set_partition(d->be, cm.rank, cm.nranks), "subtree partition")) return false; }
  else
  {
    const long M = (long)(unsigned int)ctx->Nmeasurements;
    d->row0 = (int)(M*cm.rank/cm.nranks); d->row1 = (int)(M*(cm.rank + 1)/cm.nranks);
    if(!be_ok(dlg_backend_set_shard(d->be, d->row0, d->row1, nullptr, nullptr), "row shard")) return false;
  }
  // the sums across the ranks: the process's RCCL communicator, one made from the caller's id, or the caller's hook
  bool ok;
  if(g_env_comm.ok && g_env_comm.holder && !cm.have_id && !cm.fn)
    ok = be_ok(dlg_backend_share_rccl(d->be, g_env_comm.holder), "RCCL communicator of the process");
  else if(cm.have_id) ok = be_ok(dlg_backend_init_rccl(d->be, cm.rank, cm.nranks, cm.id), "RCCL communicator");
  else if(cm.fn)      ok = be_ok(dlg_backend_set_allreduce(d->be, cm.fn, cm.cookie), "all-reduce hook");
  else { MSG("a communicator of %d ranks needs an RCCL id or an all-reduce hook", cm.nranks); ok = false; }
  d->sharded = ok;
  return ok;
}

bool one_rank_only(const char* who)
{
  if(!t_comm.set && !env_world()) return true;
  MSG("%s: one rank only (a communicator is set: dogleg_amd_clear_communicator)", who);
  return false;
}

extern "C" {

int dogleg_amd_set_communicator(int rank, int nranks, int device, const void* rccl_unique_id128)
{
  if(nranks < 1 || rank < 0 || rank >= nranks || !rccl_unique_id128) { MSG("dogleg_amd_set_communicator: bad arguments"); return -1; }
  Comm c; c.rank = rank; c.nranks = nranks; c.device = device; c.have_id = true; memcpy(c.id, rccl_unique_id128, 128); c.set = true;
  t_comm = c;
  return 0;
}
int dogleg_amd_set_allreduce(int rank, int nranks, int device, dogleg_amd_allreduce_t fn, void* cookie)
{
  if(nranks < 1 || rank < 0 || rank >= nranks || !fn) { MSG("dogleg_amd_set_allreduce: bad arguments"); return -1; }
  Comm c; c.rank = rank; c.nranks = nranks; c.device = device; c.fn = fn; c.cookie = cookie; c.set = true;
  t_comm = c;
  return 0;
}
void dogleg_amd_clear_communicator(void) { t_comm = Comm(); }

int dogleg_amd_rccl_unique_id(void* out128) { return dlg_rccl_unique_id(out128) == DLG_OK ? 0 : -1; }
int dogleg_amd_rank(const dogleg_solverContext_t* ctx, int* nranks)
{
  const Driver* d = reinterpret_cast<const Driver*>(ctx);
  if(!d) return -1;
  if(nranks) *nranks = d->sharded ? d->nranks : 1;
  return d->sharded ? d->rank : 0;
}

} // extern "C"
