// mirhi_native_flags.h -- memory scope of a native packet's acquire / release fences: what a submit picks (packet_scopes, mirhi_submit.h) and native_enqueue
// (mirhi_native.h) writes into the packet header.  Agent scope unless asked for system scope (the first kernel of a submit must see what the host wrote,
// the last one must publish the frame to the host and the copy engines; the ones in between only talk to each other: a system-scope fence on every
// packet cost the frame loop 4 - 7 %).  Plain C++, no HIP.
#pragma once
#include <stdint.h>

namespace mirhi {
enum : uint32_t { NATIVE_ACQUIRE_SYSTEM = 1u, NATIVE_RELEASE_SYSTEM = 2u };
}  // namespace mirhi
