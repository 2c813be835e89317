// sndwrite_step_lib.cpp — TEST INFRASTRUCTURE ONLY: sndwrite_step_host.hpp's
// batch loop behind one C symbol, built without a sanitizer into a temporary
// shared object that tests/test_sndwrite_model.py loads with ctypes.
#include "sndwrite_step_host.hpp"

extern "C" uint64_t sndwrite_step_batch(const mtcp_gpu_sndwrite_req *req, uint32_t n, uint32_t max_id,
                                        mtcp_gpu_ack_state *snd, mtcp_gpu_datagen_state *dtx, const uint8_t *src,
                                        uint64_t src_bytes, uint8_t *payload, uint64_t payload_bytes,
                                        mtcp_gpu_sndwrite_res *wres, uint32_t *seg_sid, uint32_t *seg_start,
                                        uint32_t *seg_stop, uint32_t *nseg, uint64_t total[2]) {
    return sndwrite_host::apply_batch(req, n, max_id, snd, dtx, src, src_bytes, payload, payload_bytes, wres, seg_sid,
                                      seg_start, seg_stop, nseg, total);
}
