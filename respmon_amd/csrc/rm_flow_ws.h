// respmon_amd/csrc/rm_flow_ws.h -- the named device buffers of the optical-flow path (rm_flow.h).  Every context embeds one (rm_ctx::flow),
// so this is the one part of that path every unit sees; its kernels and launchers are rm_motion.hip's alone.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>

#include "../../include/respmon_hip.h"

namespace rm {

struct FlowWorkspace {
    struct Buf { void *p = nullptr; size_t cap = 0; };
    std::map<std::string, Buf> bufs;
    int get(const std::string &name, size_t bytes, void **out, std::string &err)
    {
        Buf &b = bufs[name];
        if (b.cap < bytes) {
            if (b.p) (void)hipFree(b.p);
            b.p = nullptr; b.cap = 0;
            size_t cap = (bytes + 255) / 256 * 256;
            if (hipMalloc(&b.p, cap) != hipSuccess) { err = "hipMalloc failed in flow workspace"; return RM_E_NOMEM; }
            b.cap = cap;
        }
        *out = b.p;
        return RM_OK;
    }
    ~FlowWorkspace()
    {
        for (auto &kv : bufs)
            if (kv.second.p) (void)hipFree(kv.second.p);
    }
};

}  // namespace rm
