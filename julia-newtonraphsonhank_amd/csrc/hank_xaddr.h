// hank_xaddr.h — plain C++ on integers, no device code: the one predicate the host asks before it lets the Dual-pass persistent sweeps
// (hank_xsweep.h) address their streams with 32-bit offsets. A CPU test compiles this header alone
// (tests/test_xaddr_host.py).
#pragma once

namespace hank {

// Do 32-bit offsets reach every stream of a Dual-pass launch? The record and this launch's dpol ([P][groups][G][D] doubles) are
// addressed through buffer descriptors — a lane offset on top of a scalar offset, an unsigned 32-bit sum — so each must leave room
// for the largest lane offset (XADDR_MARGIN: one period of a group's dpol, G D 8 bytes, must fit in it). The work units
// ([P][members][XUCAP] int2) keep their pointer and are indexed by ONE unsigned 32-bit scalar: their bytes are held to the same limit.
constexpr unsigned long long XADDR_MARGIN = 1ull << 24;
static inline bool x_addr_fits(unsigned long long rec_bytes, unsigned long long P, unsigned long long groups, unsigned long long G, unsigned long long D,
                               unsigned long long members, unsigned long long ucap) {
    const unsigned long long lim = (1ull << 32) - XADDR_MARGIN;
    return rec_bytes <= lim && P * groups * G * D * 8ull <= lim && P * members * ucap * 8ull <= lim && G * D * 8ull <= XADDR_MARGIN;
}

}  // namespace hank
