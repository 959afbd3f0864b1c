// lisreg_api_comm.hip — the RCCL pose gather behind lisreg_comm_* / lisreg_gather_results.  Host code only.
#include "lisreg_ctx.hpp"

#include <dlfcn.h>
#include <cstring>
#include <string>

using namespace lisreg;

extern "C" {

// ---- RCCL pose gather: librccl is loaded lazily so single-GPU users never pay for it ------------
// ONE RCCL per process, and never in the global symbol scope.  A host process may carry an RCCL of its own already (a PyTorch wheel
// bundles librccl.so.1 next to ITS librocm_smi64 — soname .so.7, the system's is .so.1, so the loader keeps both): the copy already
// loaded is reused (RTLD_NOLOAD by soname); only a process without one gets the system's library, RTLD_LOCAL.  Round 3 loaded it
// RTLD_GLOBAL: the system librocm_smi64's globals then interposed those of the wheel's copy imported later, both static destructors
// freed the same std::map at exit, and glibc aborted the process ("double free or corruption", exit status 134) after every test had
// passed.  tests/test_teardown.py runs that sequence in a subprocess.
static void* rccl_dlopen()
{
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    return h;
}

static int rccl_load(lisreg_ctx* c)
{
    if (c->rccl.handle) return LISREG_OK;
    void* h = rccl_dlopen();
    if (!h) return ctx_fail(c, LISREG_ERR_COMM, std::string("dlopen(librccl.so): ") + dlerror());
    c->rccl.handle = h;
    c->rccl.GetUniqueId = (int (*)(void*))dlsym(h, "ncclGetUniqueId");
    c->rccl.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
    c->rccl.CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
    if (!c->rccl.GetUniqueId || !c->rccl.AllGather || !c->rccl.CommDestroy || !dlsym(h, "ncclCommInitRank"))
        return ctx_fail(c, LISREG_ERR_COMM, "librccl.so lacks the expected nccl* symbols");
    return LISREG_OK;
}

int lisreg_comm_unique_id(unsigned char id[128])
{
    if (!id) return LISREG_ERR_ARG;
    void* h = rccl_dlopen();                      // reference-counted by the loader; the library stays for the life of the process
    if (!h) return ctx_fail(nullptr, LISREG_ERR_COMM, "dlopen(librccl.so) failed");
    auto f = (int (*)(void*))dlsym(h, "ncclGetUniqueId");
    if (!f || f(id) != 0) return ctx_fail(nullptr, LISREG_ERR_COMM, "ncclGetUniqueId failed");
    return LISREG_OK;
}

namespace { struct UniqueId128 { char b[128]; }; }

int lisreg_comm_init(lisreg_ctx* c, int rank, int nranks, const unsigned char id[128])
{
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return LISREG_ERR_ARG;
    int rc = rccl_load(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    UniqueId128 uid;
    memcpy(uid.b, id, 128);
    auto init = (int (*)(void**, int, UniqueId128, int))dlsym(c->rccl.handle, "ncclCommInitRank");
    if (init(&c->comm, nranks, uid, rank) != 0) return ctx_fail(c, LISREG_ERR_COMM, "ncclCommInitRank failed");
    c->comm_nranks = nranks;
    return LISREG_OK;
}

int lisreg_gather_results(lisreg_ctx* c, const void* local_device, int n_local, void* out_device)
{
    if (!c || !local_device || !out_device || n_local < 0) return LISREG_ERR_ARG;
    if (!c->comm) return ctx_fail(c, LISREG_ERR_COMM, "gather_results: call lisreg_comm_init first");
    const int ncclFloat32 = 7;
    if (c->rccl.AllGather(local_device, out_device, (size_t)n_local * kResultSize, ncclFloat32, c->comm, c->stream) != 0)
        return ctx_fail(c, LISREG_ERR_COMM, "ncclAllGather failed");
    return LISREG_OK;
}

void lisreg_comm_destroy(lisreg_ctx* c)
{
    if (!c || !c->comm) return;
    if (c->rccl.CommDestroy) c->rccl.CommDestroy(c->comm);
    c->comm = nullptr;
}

}  // extern "C"
