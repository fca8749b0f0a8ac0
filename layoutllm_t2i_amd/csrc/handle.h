// Host machinery shared by the UNet handle (engine.hip, gl_engine) and the VAE handle (vae_engine.hip, gl_vae): the packed-weight
// table, the grow-only activation pool, the hipGraph cache and the per-handle option overrides.  Host-only: no kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "gligen_hip.h"
#include "opts.h"

#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#define CK(expr)                                     \
    do {                                             \
        const int rc__ = (expr);                     \
        if (rc__ != 0) return rc__;                  \
    } while (0)
#define CKP(ptr)                                     \
    do {                                             \
        if ((ptr) == nullptr) return GL_ERR_BAD_ARG; \
    } while (0)

// The LIBRARY-DEFINED flat weight layout: entries in creation order, every offset a multiple of 256 bytes.  The host packer fills the
// buffer by this table (gl_weight_at / gl_vae_weight_at); the same buffer travels in the multi-GPU broadcast.
struct gl_weight_table {
    struct Entry {
        int64_t off, bytes;
        int dtype, ndim;            // dtype 0 = fp16, 1 = fp32
        int64_t shape[4];
    };
    static constexpr int64_t ALIGN = 256;
    std::vector<std::string> names;
    std::unordered_map<std::string, Entry> tab;
    int64_t total = 0;
    const char* wbase = nullptr;    // the loaded buffer: referenced, not copied

    void add(const std::string& name, int dtype, std::initializer_list<int64_t> shape) {
        Entry w{};
        w.dtype = dtype;
        w.ndim = (int)shape.size();
        int64_t n = 1;
        int i = 0;
        for (int64_t s : shape) { w.shape[i++] = s; n *= s; }
        w.bytes = n * (dtype == 0 ? 2 : 4);
        w.off = total;
        total += (w.bytes + ALIGN - 1) / ALIGN * ALIGN;
        tab[name] = w;
        names.push_back(name);
    }
    const Entry* find(const std::string& name) const {
        auto it = tab.find(name);
        return it == tab.end() ? nullptr : &it->second;
    }
    template <typename T>
    const T* ptr(const std::string& name) const {
        const Entry* w = find(name);
        return w == nullptr || wbase == nullptr ? nullptr : reinterpret_cast<const T*>(wbase + w->off);
    }
    int info_at(int32_t i, gl_weight_info* info) const {
        if (!info || i < 0 || i >= (int)names.size()) return GL_ERR_BAD_ARG;
        const std::string& n = names[i];
        if (n.size() >= sizeof(info->name)) return GL_ERR_BAD_ARG;
        const Entry& w = tab.at(n);
        memset(info, 0, sizeof(*info));
        memcpy(info->name, n.c_str(), n.size());
        info->offset = w.off; info->nbytes = w.bytes; info->dtype = w.dtype; info->ndim = w.ndim;
        for (int k = 0; k < 4; ++k) info->shape[k] = w.shape[k];
        return 0;
    }
};

// Grow-only activation pool: one device buffer per tag, whose address is stable until a larger request replaces it (`changed`: the
// captured graphs hold the old addresses and are stale).  It never allocates while a stream capture is open.
struct gl_pool {
    struct Buf { void* p; size_t bytes; };
    std::unordered_map<std::string, Buf> bufs;
    bool changed = false, capturing = false;

    void* get(const std::string& tag, size_t bytes, std::string* err) {
        auto it = bufs.find(tag);
        if (it != bufs.end() && it->second.bytes >= bytes) return it->second.p;
        if (capturing) { if (err) *err = "pool allocation during graph capture: " + tag; return nullptr; }
        if (it != bufs.end()) { (void)hipFree(it->second.p); bufs.erase(it); }
        void* p = nullptr;
        const size_t rounded = (bytes + 255) / 256 * 256;
        if (hipMalloc(&p, rounded) != hipSuccess) { if (err) *err = "hipMalloc failed for " + tag; return nullptr; }
        bufs[tag] = Buf{p, rounded};
        changed = true;
        return p;
    }
    int64_t bytes() const {
        int64_t s = 0;
        for (auto& kv : bufs) s += (int64_t)kv.second.bytes;
        return s;
    }
    void release() {
        for (auto& kv : bufs) (void)hipFree(kv.second.p);
        bufs.clear();
    }
};

// One instantiated hipGraph per key.  Graphs are captured on a stream the cache owns (the caller's may be the legacy default stream,
// which cannot be captured) and launched on the caller's.  Besides the key a captured launch sequence depends on the pool addresses
// and on the option generation: a change of either drops every graph.
template <typename Key>
struct gl_graph_cache {
    std::map<Key, hipGraphExec_t> graphs;
    hipStream_t cap_stream = nullptr;
    int opt_epoch = 0;              // gl_set_option generation the captured graphs were built under
    int ovr_epoch = 0;              // ... and the generation of the handle's own overrides

    void drop() {
        for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
        graphs.clear();
    }
    void release() {
        drop();
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
        cap_stream = nullptr;
    }
    void sync_epochs(const gl_opt_overrides& ovr) {       // a tuning knob changed: the captured launch sequences may be stale
        if (opt_epoch == g_gl_option_epoch && ovr_epoch == ovr.epoch) return;
        drop();
        opt_epoch = g_gl_option_epoch;
        ovr_epoch = ovr.epoch;
    }
    // launch: (hipStream_t, int* n_launches) -> int, the launch sequence `key` names.  Eager on `st`, or the key's graph replayed on
    // `st`; on a cache miss a warm-up run first allocates every pooled buffer, then the same sequence is captured and replayed.
    template <typename Launch>
    int run(const Key& key, bool use_graph, hipStream_t st, gl_pool& pool, Launch launch, int* launches) {
        if (!use_graph) {
            CK(launch(st, launches));
            if (pool.changed) { drop(); pool.changed = false; }
            return 0;
        }
        auto it = graphs.find(key);
        if (it == graphs.end()) {
            CK(launch(st, launches));
            if (hipStreamSynchronize(st) != hipSuccess) return GL_ERR_BAD_ARG;
            if (pool.changed) { drop(); pool.changed = false; }
            hipGraph_t graph = nullptr;
            if (cap_stream == nullptr && hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking) != hipSuccess) return GL_ERR_UNSUPPORTED;
            if (hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return GL_ERR_UNSUPPORTED;
            pool.capturing = true;
            const int rc = launch(cap_stream, nullptr);
            pool.capturing = false;
            const hipError_t ec = hipStreamEndCapture(cap_stream, &graph);
            if (rc != 0 || ec != hipSuccess || graph == nullptr) {
                if (graph) (void)hipGraphDestroy(graph);
                return rc != 0 ? rc : GL_ERR_UNSUPPORTED;
            }
            hipGraphExec_t exec = nullptr;
            const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (ei != hipSuccess) return GL_ERR_UNSUPPORTED;
            it = graphs.emplace(key, exec).first;
        }
        return hipGraphLaunch(it->second, st) == hipSuccess ? 0 : GL_ERR_UNSUPPORTED;
    }
};

// gl_set_handle_option / gl_vae_set_option: the value is normalised exactly like the process-level setter's
static inline int gl_handle_set_option(gl_opt_overrides& ovr, int key, int value) {
    gl_opts probe{};
    if (key < 0 || key >= GL_OPT_MAX || !gl_opts_put(probe, key, value)) return GL_ERR_BAD_ARG;
    ovr.mask |= (uint64_t)1 << key;
    ovr.v[key] = value;
    ++ovr.epoch;
    return 0;
}
