// comm.hip -- multi-GPU: the sharded path's one collective, on RCCL loaded at run time.
#include <string.h>

#include <mutex>

#include <dlfcn.h>

#include "exec.h"

using namespace sbbseg;

namespace {

// ---- RCCL, loaded at run time: libsbbseg has no link-time dependency on librccl (it must load on a box without it, and
// on the CPU-only build container); the sharded path's one collective is the all-gather of u8 label maps
struct RcclUniqueId { char internal[128]; };                  // = ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES 128)
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(RcclUniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, RcclUniqueId, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;
std::mutex g_rccl_mutex;                                      // (handles on distinct devices may be driven from distinct threads)
int rccl_load()
{
    std::lock_guard<std::mutex> lock(g_rccl_mutex);
    if (g_rccl.lib) return 0;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names)
        if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    REQUIRE(h, "librccl not found (tried librccl.so.1, librccl.so, /opt/rocm/lib/librccl.so.1): %s", dlerror());
    RcclApi a;
    a.GetUniqueId = (int (*)(RcclUniqueId*))dlsym(h, "ncclGetUniqueId");
    a.CommInitRank = (int (*)(void**, int, RcclUniqueId, int))dlsym(h, "ncclCommInitRank");
    a.CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
    a.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
    a.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllGather || !a.GetErrorString) {
        dlclose(h);
        return set_error("librccl lacks an expected symbol (ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllGather)");
    }
    a.lib = h;
    g_rccl = a;
    return 0;
}
#define RCCLCHK(expr)                                                                              \
    do {                                                                                           \
        const int r_ = (expr);                                                                     \
        if (r_ != 0) return set_error("%s failed: %s", #expr, g_rccl.GetErrorString(r_));          \
    } while (0)

}  // namespace

namespace sbbseg {

void comm_release(sbbseg_ctx* c)
{
    if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
    c->comm = nullptr; c->comm_rank = 0; c->comm_world = 1;
}

}  // namespace sbbseg

extern "C" {

// ------------------------------------------------------------------------------ multi-GPU: the one collective, on RCCL
int sbbseg_comm_unique_id(char* id128)
{
    API_BEGIN
    REQUIRE(id128, "bad arguments");
    if (rccl_load()) return 1;
    RcclUniqueId id;
    RCCLCHK(g_rccl.GetUniqueId(&id));
    memcpy(id128, id.internal, sizeof(id.internal));
    return 0;
    API_END
}

int sbbseg_comm_init(sbbseg_ctx* c, int rank, int world, const char* id128)
{
    API_BEGIN
    REQUIRE(c && id128 && world >= 1 && rank >= 0 && rank < world, "bad arguments (rank %d of %d)", rank, world);
    HIPCHK(hipSetDevice(c->device));
    if (rccl_load()) return 1;
    comm_release(c);
    RcclUniqueId id;
    memcpy(id.internal, id128, sizeof(id.internal));
    void* comm = nullptr;
    RCCLCHK(g_rccl.CommInitRank(&comm, world, id, rank));
    c->comm = comm; c->comm_rank = rank; c->comm_world = world;
    return 0;
    API_END
}

int sbbseg_comm_info(sbbseg_ctx* c, int* rank, int* world)
{
    API_BEGIN
    REQUIRE(c && rank && world, "bad arguments");
    *rank = c->comm_rank; *world = c->comm ? c->comm_world : 0;
    return 0;
    API_END
}

int sbbseg_comm_destroy(sbbseg_ctx* c)
{
    API_BEGIN
    REQUIRE(c, "null handle");
    comm_release(c);
    return 0;
    API_END
}

int sbbseg_allgather_labels_dev(sbbseg_ctx* c, const void* d_send, size_t bytes_per_rank, void* d_recv)
{
    API_BEGIN
    REQUIRE(c && d_send && d_recv, "bad arguments");
    REQUIRE(c->comm, "no communicator: call sbbseg_comm_init first");
    HIPCHK(hipSetDevice(c->device));
    if (bytes_per_rank == 0) return 0;
    RCCLCHK(g_rccl.AllGather(d_send, d_recv, bytes_per_rank, /* ncclUint8 */ 1, c->comm, c->stream));
    return 0;
    API_END
}

}  // extern "C"
