// rcvread_step_lib.cpp — TEST INFRASTRUCTURE ONLY: rcvread_step_host.hpp's
// batch loop behind one C symbol, built without a sanitizer into a temporary
// shared object that tests/test_rcvread_model.py loads with ctypes.
#include "rcvread_step_host.hpp"

extern "C" uint64_t rcvread_step_batch(const mtcp_gpu_rcvread_req *req, uint32_t n, uint32_t max_id,
                                       mtcp_gpu_rcv_state *state, mtcp_gpu_rcv_buf *rbuf, mtcp_gpu_ackgen_state *tx,
                                       const mtcp_gpu_ack_state *snd, const uint8_t *arena, uint64_t arena_bytes,
                                       uint8_t *dst, uint64_t dst_bytes, mtcp_gpu_rcvread_res *rres,
                                       uint64_t total[2]) {
    return rcvread_host::apply_batch(req, n, max_id, state, rbuf, tx, snd, arena, arena_bytes, dst, dst_bytes, rres,
                                     total);
}
