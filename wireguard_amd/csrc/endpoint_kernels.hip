// endpoint_kernels.hip -- the peer endpoints on device-resident tables
// (include/wgcsum.h): the bodies of wgcs_endpoint.h under the one kernel of
// wgcs_each.h, instantiated below:
//   EndpointRecv            the endpoint of every slot of a receive batch         bind.go:308-319
//   SetEndpointFromPacket behind write_build, accept and finish                   peer.go:281-286
//     EndpointSetClaim      every candidate claims its peer's row
//     EndpointSetCommit     the holder, the highest candidate of its peer, stores its 64 bytes
//   Peer.Send up to bind.Send for jobs, initiations and responses                 peer.go:201-211
//     EndpointDstRead       destination, family and status of every entry (EndpointDstJobs: and a job's bytes)
//     EndpointDstClear      ClearSrc on the table rows whose flag was set
// The set and dst bodies are templated on the source that turns an index into
// a peer row (wgcs_events.h).  A recv lane walks at most a few control
// messages of its own slot in aligned words and stores one 64-byte row; a set
// or dst lane is two or three dependent loads, one 32-bit atomic and at most one
// row.  No kernel reads a clock or allocates.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_each.h"
#include "wgcs_endpoint.h"
#include "wgcs_kernels.h"

namespace wgcs {

template hipError_t launch_each(const EndpointRecv&, uint32_t, hipStream_t);
template hipError_t launch_each(const EndpointSetClaim<GroupRows>&, const EndpointSetCommit<GroupRows>&, uint32_t,
                                hipStream_t);
template hipError_t launch_each(const EndpointSetClaim<AcceptedRows>&, const EndpointSetCommit<AcceptedRows>&, uint32_t,
                                hipStream_t);
template hipError_t launch_each(const EndpointSetClaim<FinishedRows>&, const EndpointSetCommit<FinishedRows>&, uint32_t,
                                hipStream_t);
template hipError_t launch_each(const EndpointDstJobs&, const EndpointDstClear<KeptJobRows>&, uint32_t, hipStream_t);
template hipError_t launch_each(const EndpointDstRead<InitiatedRows>&, const EndpointDstClear<InitiatedRows>&, uint32_t,
                                hipStream_t);
template hipError_t launch_each(const EndpointDstRead<RespondedRows>&, const EndpointDstClear<RespondedRows>&, uint32_t,
                                hipStream_t);

}  // namespace wgcs
