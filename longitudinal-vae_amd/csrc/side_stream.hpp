// side_stream.hpp -- the one high-priority side stream (per device) on which the blocked inverse
// (chol_inv.hip) runs its critical chain of pivot-block kernels beside the bulk updates,
// and the early stream the caller may LEND (lvae_set_early_stream), on which chol_inv.hip starts the part of
// trtri that needs only the first block columns beside potrf's pivot-bound tail.  The library creates no
// second stream of its own: a process here has 4 hardware queues, and a fifth stream of the step serialises
// with another one (measured: 8.6 -> 11.1-11.5 ms per closed step from creating it alone).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

namespace lvae {

struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, prep = nullptr, c = nullptr, u2p[2] = {}, piv[2] = {};
  hipEvent_t rbx = nullptr, rb = nullptr;  // the binned residual's plan (kl_closed.hip): x ready / plan done
  hipStream_t early = nullptr;             // lent by the caller or null: trtri's early part (chol_inv.hip)
  hipEvent_t efork = nullptr, edone = nullptr;  // its fork (the caller's stream after panel(s-1)) and join
  int cus = 0;                             // compute units of the device (the early launches' grid cap)
};

// Held for a call's whole enqueue sequence (every record / wait on the side streams and their events);
// recursive: the exact KL's factor call holds it around the inverse's own sequence.
std::recursive_mutex& side_mutex();
// The current device's side stream and events, created together on first use (never later: not inside a
// stream capture that began after a warm-up call) and kept for the process lifetime: ONE set per device,
// shared by every caller stream (calls from different caller streams serialise on it; the enqueue
// sequences cannot interleave under side_mutex()).  0 or LVAE_ERR_LAUNCH.
int side_stream(SideStream*& out);

}  // namespace lvae
