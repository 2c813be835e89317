// sndwrite_step_host.hpp — TEST INFRASTRUCTURE ONLY: mtcp_gpu_sndwrite_dev's
// launches as a plain host loop around the text the plan kernel runs
// (mtcp_amd/csrc/sndwrite_step.hpp): the claim, write_step per request with the
// loads and stores sndwrite_plan_kernel makes, then every move as a memmove
// and every copy as a memcpy.  tests/c/sndwrite_step_test.cpp (under the
// sanitizers) and tests/c/sndwrite_step_lib.cpp (loaded by
// tests/test_sndwrite_model.py) use it.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../mtcp_amd/csrc/sndwrite_step.hpp"

namespace sndwrite_host {

// Returns the batch's copy units (what the scan's total would be).
inline uint64_t apply_batch(const mtcp_gpu_sndwrite_req *req, uint32_t n, uint32_t max_id, mtcp_gpu_ack_state *snd,
                            mtcp_gpu_datagen_state *dtx, const uint8_t *src, uint64_t src_bytes, uint8_t *payload,
                            uint64_t payload_bytes, mtcp_gpu_sndwrite_res *wres, uint32_t *seg_sid,
                            uint32_t *seg_start, uint32_t *seg_stop, uint32_t *nseg, uint64_t total[2]) {
    // clear and claim: "none" at the requests' sids only, then the minimum index
    std::vector<uint32_t> claim((size_t)max_id + 1, 0xA5A5A5A5u);
    for (uint32_t i = 0; i < n; ++i)
        if (req[i].sid <= max_id) claim[req[i].sid] = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i)
        if (req[i].sid <= max_id && i < claim[req[i].sid]) claim[req[i].sid] = i;
    total[0] = total[1] = 0;
    uint64_t units = 0;
    std::vector<mg::WriteOut> outs(n);
    for (uint32_t i = 0; i < n; ++i) {
        mg::WriteIn in{};
        memcpy(in.req, &req[i], 32);
        in.max_id = max_id, in.src_bytes = src_bytes, in.payload_bytes = payload_bytes;
        const uint32_t sid = req[i].sid;
        if (sid <= max_id) {
            uint32_t s[32], d[4];
            memcpy(s, &snd[sid], 128), memcpy(d, &dtx[sid], 16);
            in.snd_wnd = s[2], in.sb_head_seq = s[16], in.sb_len = s[17], in.sb_size = s[18], in.mss2 = s[19];
            in.bits = s[20], in.bits2 = s[21];
            in.sb_off = (uint64_t)d[1] << 32 | d[0], in.sb_base_seq = d[2], in.dflags = d[3];
            in.dup = claim[sid] != i;
        }
        const mg::WriteOut o = outs[i] = mg::write_step(in);
        if (o.st_wnd) snd[sid].snd_wnd = o.snd_wnd;
        if (o.st_rec) snd[sid].sb_len = o.sb_len, dtx[sid].sb_base_seq = o.sb_base_seq, dtx[sid].on_send_list = 1;
        memcpy(&wres[i], o.res, 16);
        seg_sid[i] = o.st_rec ? sid : MTCP_GPU_FLOW_NONE;
        seg_start[i] = 0, seg_stop[i] = 0;
        if (o.to_put) total[0] += 1, total[1] += o.to_put, units += mg::write_units(o.dst, o.to_put);
    }
    if (n) seg_start[n] = 0, nseg[0] = n;
    for (uint32_t i = 0; i < n; ++i)
        if (outs[i].move_len) {
            const uint64_t to = outs[i].dst - outs[i].move_len;
            memmove(payload + to, payload + to + outs[i].head_off, outs[i].move_len);
        }
    for (uint32_t i = 0; i < n; ++i)
        if (outs[i].to_put) memcpy(payload + outs[i].dst, src + outs[i].src, outs[i].to_put);
    return units;
}

}  // namespace sndwrite_host
