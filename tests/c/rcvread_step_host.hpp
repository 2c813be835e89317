// rcvread_step_host.hpp — TEST INFRASTRUCTURE ONLY: mtcp_gpu_rcvread_dev's
// launches as a plain host loop around the text the plan kernel runs
// (mtcp_amd/csrc/rcvread_step.hpp): the claim, read_step per request with the
// loads and stores rcvread_plan_kernel makes, and the copy as a memcpy.
// tests/c/rcvread_step_test.cpp (under the sanitizers) and
// tests/c/rcvread_step_lib.cpp (loaded by tests/test_rcvread_model.py) use it.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../mtcp_amd/csrc/rcvread_step.hpp"

namespace rcvread_host {

// Returns the batch's copy units (what the scan's total would be).
inline uint64_t apply_batch(const mtcp_gpu_rcvread_req *req, uint32_t n, uint32_t max_id, mtcp_gpu_rcv_state *state,
                            mtcp_gpu_rcv_buf *rbuf, mtcp_gpu_ackgen_state *tx, const mtcp_gpu_ack_state *snd,
                            const uint8_t *arena, uint64_t arena_bytes, uint8_t *dst, uint64_t dst_bytes,
                            mtcp_gpu_rcvread_res *rres, uint64_t total[2]) {
    // clear and claim: "none" at the requests' sids only, then the minimum index
    std::vector<uint32_t> claim((size_t)max_id + 1, 0xA5A5A5A5u);
    for (uint32_t i = 0; i < n; ++i)
        if (req[i].sid <= max_id) claim[req[i].sid] = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i)
        if (req[i].sid <= max_id && i < claim[req[i].sid]) claim[req[i].sid] = i;
    total[0] = total[1] = 0;
    uint64_t units = 0;
    for (uint32_t i = 0; i < n; ++i) {
        mg::ReadIn in{};
        memcpy(in.req, &req[i], 32);
        in.max_id = max_id, in.arena_bytes = arena_bytes, in.dst_bytes = dst_bytes;
        const uint32_t sid = req[i].sid;
        if (sid <= max_id) {
            memcpy(in.st, &state[sid], 64);
            memcpy(in.rb, &rbuf[sid], 32);
            in.has_tx = tx != nullptr;
            if (in.has_tx) in.need_wnd_adv = tx[sid].need_wnd_adv, in.eff_mss = snd[sid].eff_mss;
            in.dup = claim[sid] != i;
        }
        const mg::ReadOut o = mg::read_step(in);
        if (o.st_rec) {
            memcpy(&state[sid], o.st, 64);
            rbuf[sid].head_offset = o.rb_head, rbuf[sid].last_len = o.rb_last;
        }
        if (o.st_tx) tx[sid].need_wnd_adv = 0;
        memcpy(&rres[i], o.res, 16);
        if (o.copylen) {
            memcpy(dst + req[i].dst_off, arena + o.src, o.copylen);
            total[0] += 1, total[1] += o.copylen;
            units += mg::read_units(req[i].dst_off, o.copylen);
        }
    }
    return units;
}

}  // namespace rcvread_host
