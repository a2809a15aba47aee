// cookiegen_kernels.hip -- the initiator's side of the cookie mechanism on
// device-resident tables (include/wgcsum.h): the bodies of wgcs_cookiegen.h
// under the one kernel of wgcs_each.h, instantiated below:
//   lastMAC1 behind initiate and respond                        cookie.go:301-302
//     CookieSentClaim     every descriptor that takes part claims its peer's row
//     CookieSentCommit    the holder, the highest descriptor of its peer, stores its MAC1
//   cookie replies over a receive batch                         receive.go:246-269, cookie.go:319-339
//     CookieOpen          lookup, XChaCha20-Poly1305 open, the cookie into d_work, the claim
//     CookieCommit        the holder stores cookie, bit and time; d_work is zeroed
//   CookieAge             CookieRefreshTime over the peer rows   cookie.go:306
// An open lane is two dependent slot probes, one HChaCha20, two ChaCha20 blocks
// and a three-block Poly1305 on registers (wgcs_xchacha.h: nothing is indexed
// at run time), 64 bytes in -- replies sit at any offset; b2s_load_block reads
// the aligned dwords that hold them -- and 16 bytes out.  The kernels read the
// arena and never write it, draw no randomness and read no clock.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_cookiegen.h"
#include "wgcs_each.h"
#include "wgcs_kernels.h"

namespace wgcs {

template hipError_t launch_each(const CookieSentClaim<InitiatedRows>&, const CookieSentCommit<InitiatedRows>&, uint32_t,
                                hipStream_t);
template hipError_t launch_each(const CookieSentClaim<RespondedRows>&, const CookieSentCommit<RespondedRows>&, uint32_t,
                                hipStream_t);
template hipError_t launch_each(const CookieOpen&, const CookieCommit&, uint32_t, hipStream_t);
template hipError_t launch_each(const CookieAge&, uint32_t, hipStream_t);

}  // namespace wgcs
