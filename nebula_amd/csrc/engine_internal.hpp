// engine_internal.hpp — what engine.cpp offers window.cpp and queue.cpp beside the C ABI
// (include/nebula_aead.h): hidden symbols, declared here once, described at their definitions.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>

#include "../../include/nebula_aead.h"
#include "sched.hpp"
#include "workspace.hpp"  // (and hip_owned.hpp)

struct SchedSpace;  // the mixed-key scheduler's device workspace

extern "C" {
int neb_engine_device_of(const neb_engine* e);
int neb_check_batch_args(neb_engine* e, int alg, uint32_t key_hint);
int neb_key_alg(neb_engine* e, uint32_t key);
bool neb_host_mapped(const void* p);
void neb_engine_key_table(const neb_engine* e, const uint32_t** d_keys, uint32_t* max_keys);
SchedSpace* neb_sched_space_new();
void neb_sched_space_free(SchedSpace* sp);  // with the engine's device current
int neb_launch_on(neb_engine* e, int alg, int open, const neb_desc* desc, uint32_t n, uint8_t* arena,
                  int32_t* status, uint32_t key_hint, hipStream_t s, SchedSpace* sched);
int neb_open_batch_count(neb_engine* e, int alg, const neb_desc* d_desc, uint32_t n, const uint32_t* d_n,
                         uint8_t* d_arena, int32_t* d_status, uint32_t key_hint, hipStream_t s, const uint8_t* rx,
                         SchedSpace* prebinned);
int neb_seal_batch_count(neb_engine* e, int alg, const neb_desc* d_desc, uint32_t n, const uint32_t* d_n,
                         uint8_t* d_arena, int32_t* d_status, uint32_t key_hint, hipStream_t s);
int neb_rx_sched_begin(neb_engine* e, uint32_t n, SchedSpace* sched, hipStream_t s, neb::SchedWs* ws,
                       uint32_t* max_keys);
void neb_rx_sched_abort(SchedSpace* sched);
bool neb_rx_pipe_begin(neb_engine* e, int alg, uint32_t key_hint, uint8_t* arena, uint32_t n, uint32_t nchunks,
                       neb_desc** h_desc, int32_t** h_status, int* rc);
int neb_rx_pipe_submit(neb_engine* e, int alg, uint32_t key_hint, uint8_t* arena, uint32_t c0, uint32_t cnt,
                       uint32_t k);
int neb_rx_pipe_wait(neb_engine* e, uint32_t k);
void neb_rx_pipe_end(neb_engine* e);
}

struct SchedSpaceFree {
    void operator()(SchedSpace* sp) const { neb_sched_space_free(sp); }
};
using SchedSpacePtr = std::unique_ptr<SchedSpace, SchedSpaceFree>;  // (neb_sched_space_new())
