// engine/model_tp.cpp -- tensor parallelism: the slice configuration and the peer exchange (see model.h)
#include "model_impl.h"

namespace nt {

// ---- tensor parallelism: slices ---------------------------------------------------------------------------------------------
int Model::tp_configure(int rank, int world) {
    if (world < 1 || world > 8 || rank < 0 || rank >= world) { err_ = "bad tensor-parallel rank / world"; return NTK_E_SHAPE; }
    if (!layers_.empty()) { err_ = "tp_configure must precede load"; return NTK_E_SHAPE; }
    tp_rank_ = rank;
    tp_world_ = world;
    return NTK_OK;
}

int Model::tp_check_shapes() {
    if (tp_world_ == 1) return NTK_OK;
    if (cfg_.n_heads % tp_world_ || cfg_.n_kv_heads % tp_world_ || cfg_.intermediate_size % tp_world_) {
        err_ = "heads / KV heads / FFN width do not divide over the tensor-parallel ranks";
        return NTK_E_SHAPE;
    }
    return NTK_OK;
}

int Model::tp_export(void* handle64, void** raw) {
    if (!tp_comm_) return NTK_E_NULL;
    if (raw) *raw = tp_comm_;
    if (handle64) return ntk_ipc_export(tp_comm_, handle64);
    return NTK_OK;
}

int Model::tp_connect(const void* handles, void* const* raws) {
    if (tp_world_ == 1) { tp_connected_ = true; return NTK_OK; }
    if (!tp_comm_ || (!handles && !raws)) return NTK_E_NULL;
    for (int r = 0; r < tp_world_; ++r) {
        if (r == tp_rank_) { tp_peers_[r] = tp_comm_; continue; }
        if (raws) { tp_peers_[r] = raws[r]; continue; }
        void* p = nullptr;
        const int st = ntk_ipc_open(static_cast<const uint8_t*>(handles) + 64 * r, &p);
        if (st != NTK_OK) { err_ = "mapping a peer's communication buffer failed (hipIpcOpenMemHandle)"; return st; }
        tp_peers_[r] = p;
        tp_peer_opened_[r] = true;
    }
    for (int r = 0; r < tp_world_; ++r)
        if (!tp_peers_[r]) return NTK_E_NULL;
    tp_connected_ = true;
    return NTK_OK;
}

unsigned Model::tp_error() {
    if (!tp_comm_) return 0u;
    unsigned v = 0;   // read on the model's own stream (no legacy-stream traffic next to another rank's capture)
    if (ntk_memcpy_d2h_async(&v, static_cast<uint8_t*>(tp_comm_) + 128, 4, stream_) != NTK_OK || ntk_stream_synchronize(stream_) != NTK_OK) return ~0u;
    return v;
}
float* Model::tp_slot() const { return ntk_tp_slot(tp_comm_, tp_max_floats_, tp_call_); }
int Model::tp_allreduce(float* hidden, int n) {
    if (!tp_connected_) { err_ = "tensor-parallel ranks are not connected (tp_connect)"; return NTK_E_NULL; }
    const int st = ntk_tp_allreduce_add(hidden, tp_peers_, tp_rank_, tp_world_, tp_max_floats_, tp_call_, n, stream_);
    ++tp_call_;
    return st;
}

// A tensor-parallel exchange whose bounded wait for a peer gave up has added garbage: surface it (and clear the sticky word)
int Model::check_tp() {
    if (tp_world_ <= 1 || !tp_comm_) return NTK_OK;
    const unsigned e = tp_error();
    if (e == 0u) return NTK_OK;
    const unsigned zero = 0u;
    (void)ntk_memcpy_h2d_async(static_cast<uint8_t*>(tp_comm_) + 128, &zero, 4, stream_);
    (void)ntk_stream_synchronize(stream_);
    err_ = "tensor-parallel exchange: a peer rank did not arrive (call tag " + std::to_string(e) + "); the token's results are invalid";
    fprintf(stderr, "%s\n", err_.c_str());
    return NTK_E_LAUNCH;
}

}  // namespace nt
