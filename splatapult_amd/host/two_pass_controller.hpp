// two_pass_controller.hpp -- should this Render run as two passes (csrc/msplat_occlusion.hip.h), and with what share of the visible
// splats in pass 1?  Host policy only: plain C++17, no HIP.  Its inputs are a few facts about the frame and a snapshot of what
// EARLIER two-pass frames of the context left in host-mapped memory (never waited for); any answer gives the same pixels.
// msplat_device.hip (occlusion_plan) calls decide, allocates the pass buffers, then commit; tests/sanitize/host_sanitize_driver.cpp
// replays the controller's long paths on the CPU (make sanitize).
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/msplat.h"

namespace msplat {

constexpr uint64_t kTwoPassMinSplats = 1u << 18;
constexpr uint32_t kTwoPassMinVisibleSerial = 1500000u;
constexpr float kOccFracMin = 1.0f / 256.0f, kOccFracMax = 0.75f;

// what the controller is told about the frame
struct TwoPassFrame {
    int mode;             // MSPLAT_TWO_PASS_*
    bool eligible;        // the context and the frame allow two passes at all (occlusion_plan)
    bool in_flight;       // MSPLAT_FRAMES_IN_FLIGHT (false: one frame at a time)
    uint64_t splats;      // in the cloud
    uint32_t visible;     // V of the latest frame (a host-mapped word as well)
    uint64_t bins;        // of the frame, > 0 when eligible
};

// feedback of an earlier two-pass frame: the host-mapped words kHostPass1Pairs, kHostUnfinishedBins, kHostPass2Pairs and the
// numbers of the frames the words of pass 1 / pass 2 describe (kHostPass1Seq, kHostPass2Seq)
struct TwoPassFeedback {
    uint32_t pairs1, unfinished, pairs2, seq1, seq2;
};

struct TwoPassController {
    enum { OFF = 0, PROBE = 1, WAIT = 2, ON = 3 };   // AUTO: one pass, probing (probe_left frames), waiting for the probe's feedback, two passes
    float share = 0.15f;                 // of the visible splats that goes into pass 1 (0.15-0.3 is the optimum of the blobs, 0.02 of a camera inside a scene)
    uint32_t seq = 0, change_seq = 0;    // number of the latest two-pass frame; first frame that ran with the current share
    uint32_t off = 0;                    // AUTO: frames left of a single-pass period after two passes did not pay
    uint32_t strikes = 0, backoff = 1024;   // ... decided after three looks; the pause doubles every time
    int state = OFF;
    uint32_t probe_left = 0, no_shrink = 0, wait_frames = 0;
    bool pinned = false;                 // msplat_debug_two_pass: the share is fixed
    uint64_t frames_rendered = 0;

    // msplat_debug_two_pass: share > 0 fixes the share, 0 hands it back to the controller
    void pin(float s)
    {
        pinned = s > 0.0f;
        if (pinned) share = s;
    }

    // Advances the controller by one Render.  true: two passes, with `share`; the caller then allocates what they need and calls
    // commit.  A decision that is not committed leaves seq alone (a consumed probe frame stays consumed).
    bool decide(const TwoPassFrame& f, const TwoPassFeedback& fb)
    {
        frames_rendered++;
        if (f.mode == MSPLAT_TWO_PASS_OFF || !f.eligible) return false;
        const bool forced = f.mode == MSPLAT_TWO_PASS_ON;
        if (!forced && (f.splats < kTwoPassMinSplats || frames_rendered <= 8)) return false;
        // one frame at a time and few visible splats (a rank of a row-sharded frame, a 1 M-splat cloud): the nine extra launches
        // are latency the skipped work does not buy back (rank 3 of 8 of config 4, V = 1 M: 0.33 -> 0.38 ms; with frames in flight
        // the same rank gains 12 %)
        if (!forced && !f.in_flight && f.visible < kTwoPassMinVisibleSerial) return false;

        // Only a frame that ran with the CURRENT share is evidence -- the host may be a hundred frames ahead of the GPU.
        const bool fresh = fb.seq1 == fb.seq2 && fb.seq1 != 0u && (int32_t)(fb.seq1 - change_seq) >= 0 && fb.pairs1 != 0u;
        const float ratio = fresh ? (float)fb.pairs2 / (float)fb.pairs1 : 0.0f;
        const float ufrac = fresh ? (float)fb.unfinished / (float)f.bins : 0.0f;
        if (forced) {
            if (fresh && !pinned) steer(ratio);
            return true;
        }
        // AUTO.  A bin pass 1 does not finish costs a second look; where a third of the bins never saturate whatever the share
        // (a cloud seen from outside: its rim) and the cloud is small, the nine extra launches cost what the skipped splats save
        // (BASELINE config 2: 5830 -> 5770 frames/s at best, serial 0.27 -> 0.33 ms).  So two passes are PROBED: four frames,
        // then one pass again until their feedback is in (the probe must not cost a hundred slow frames because the host runs
        // ahead); more than 30 % unfinished is a strike (the next probe takes a larger share), three strikes a pause that doubles
        // every time; otherwise two passes stay on, steered, until three looks in a row say otherwise.
        if (state == OFF) {
            if (off != 0u) { --off; return false; }
            state = PROBE;
            probe_left = 4u;
            strikes = 0u;
            set_share(0.15f);
        }
        if (state == WAIT) {
            if (!fresh) {
                // feedback that never becomes fresh (the probe frames binned nothing: the camera looked away from the cloud):
                // back to one pass with the usual pause instead of waiting for ever
                if (++wait_frames > 256u) {
                    wait_frames = 0u;
                    state = OFF;
                    off = backoff;
                }
                return false;
            }
            wait_frames = 0u;
            if (ufrac > 0.3f) {
                if (!strike()) return false;
                state = PROBE;
                probe_left = 4u;
            } else {
                state = ON;
                strikes = 0u;
                backoff = 1024u;
                steer(ratio);
            }
        } else if (state == ON && fresh && !pinned) {
            if (ufrac > 0.3f) {
                if (!strike()) return false;
            } else {
                strikes = 0u;
                steer(ratio);
            }
        }
        if (state == PROBE) {
            if (probe_left == 0u) {
                state = WAIT;
                wait_frames = 0u;
                return false;
            }
            --probe_left;
        }
        return true;
    }

    // the decided frame does run in two passes: its number (never 0)
    void commit()
    {
        if (++seq == 0u) seq = 1u;
    }

private:
    void set_share(float next)
    {
        share = std::min(kOccFracMax, std::max(kOccFracMin, next));
        change_seq = seq + 1u;           // the first frame that runs with it
    }
    // the share: pass 2 should stay well below pass 1 (a flat optimum: tools/occlusion_potential.py)
    void steer(float ratio)
    {
        // (the step from "pass 2 has nothing to do" to "pass 2 does most of the work" can be one notch: after growing, the share
        //  is not shrunk again for 32 looks)
        if (ratio > 0.6f) {
            set_share(share * 1.25f);
            no_shrink = 32u;
        } else if (no_shrink != 0u) {
            --no_shrink;
        } else if (ratio < 0.02f && share > kOccFracMin) {
            set_share(share * 0.75f);          // nothing left for pass 2: too much in pass 1
        } else if (ratio < 0.15f && share > kOccFracMin) {
            set_share(share * 0.85f);
        }
    }
    // more than 30 % unfinished.  false: the third strike, one pass for a pause that doubles every time
    bool strike()
    {
        if (++strikes >= 3u) {
            state = OFF;
            off = backoff;
            backoff = std::min(backoff * 2u, 16384u);
            return false;
        }
        set_share(share * 1.5f);
        return true;
    }
};

}  // namespace msplat
