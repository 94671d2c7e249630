// hank_xlds.h — plain C++ on integers, no device code: the dynamic-LDS layout of every persistent sweep (hank_xsweep.h), stated ONCE.
// The kernel takes its pointers from the struct, the host takes `bytes` from the same struct (x_lds_*): a carve cannot outgrow the
// size it was launched with, nor reach ctl[] — the group placement and a vote's outcome — behind it. A CPU test compiles this header
// alone (tests/test_xlds_host.py): order, lengths, alignment, and `bytes` against the formulas the schedule decisions were tuned on.
// Offsets are bytes from the start of the dynamic LDS (16-byte aligned). Pieces of doubles sit on multiples of 8; a piece read or
// written 16 bytes at a time (a tile of >= 2 slots, aggsh, xsh and dxsh of the Dual pass) on a multiple of 16; ctl is the last piece.
#pragma once
#include <cstddef>

#ifdef __HIPCC__
#define XLDS_HD __host__ __device__
#else
#define XLDS_HD
#endif

namespace hank {

constexpr size_t XCTL_BYTES = 64;      // ctl[] at the end of every persistent kernel's LDS carve: the group placement and a vote's outcome

// slots of the tangent tile: D, padded where a lane stride of 8*D bytes would bank-conflict the 16-byte reads (D = 4: 32 B
// -> lanes i and i+8 collide, 31 % of the LDS cycles in profiles/r02a; 48 B is conflict-free)
template <int D> struct XTileT { static constexpr int SL = D == 4 ? 6 : (D == 8 ? 10 : D); };
XLDS_HD inline int xtile_sl(int D) { return D == 1 ? XTileT<1>::SL : (D == 2 ? XTileT<2>::SL : XTileT<4>::SL); }      // the trait at a run-time D in {1, 2, 4}

// slots of a sweep that carries NSL numbers per grid point (the D partials and, in a Dual pass, the value)
template <int NSL> struct XSlots {
    static constexpr int SP = NSL == 1 ? 1 : ((NSL + 1) / 2) * 2;        // slots of a state row (planes of 16-byte pairs)
    static constexpr int SL = NSL <= 2 ? NSL : (NSL <= 6 ? 6 : 10);      // slots of a tile entry (see XTileT)
};
struct XSlotsRt { int SP, SL; };                                          // the traits at a run-time NSL in {1, ..., 5} (the host's size functions and buffers)
template <int NSL> constexpr XSlotsRt xslots_of() { return {XSlots<NSL>::SP, XSlots<NSL>::SL}; }
XLDS_HD inline XSlotsRt xslots(int NSL) { return NSL == 1 ? xslots_of<1>() : NSL == 2 ? xslots_of<2>() : NSL == 3 ? xslots_of<3>() : NSL == 4 ? xslots_of<4>() : xslots_of<5>(); }

// A piece of `count` elements (pads included) of `size` bytes at the next free byte; ctl is the last piece of every layout. Offsets are counted in 32 bits (LDS
// addresses are: from 64-bit integers they cost k_xdual_back scalar registers and 1 % of its time), `bytes`, which the host compares with the device's limit at ANY shape, apart in 64
struct XLdsCursor { unsigned o; size_t bytes; };
XLDS_HD inline unsigned xlds_take(XLdsCursor &k, size_t count, size_t size) { const unsigned at = k.o; k.o += (unsigned)count * (unsigned)size; k.bytes += count * size; return at; }
template <class L> XLDS_HD inline L xlds_end(L l, XLdsCursor k) { l.ctl = k.o; l.bytes = k.bytes + XCTL_BYTES; return l; }

struct XLdsPrimalBack { unsigned Vsh, Pish, ash, xsh, ctl; size_t bytes; };
XLDS_HD inline XLdsPrimalBack xlds_primal_back(int n_e, int n_a, int P) {      // it grows with the horizon P
    XLdsCursor o = {0, 0}; XLdsPrimalBack L;
    L.Vsh = xlds_take(o, (size_t)n_e * 64, 8);               // [n_e][64]
    L.Pish = xlds_take(o, (size_t)n_e * n_e, 8);             // [n_e*n_e] (registers for it would spill the 1024-thread variant)
    L.ash = xlds_take(o, n_a, 8);                            // [n_a]: the wealth grid (the bracket's grid values are a dependent load)
    L.xsh = xlds_take(o, 4 * (size_t)P, 8);                  // [P][4]: r_t, w_t, tr_t, rho_t — a cold uniform load per period otherwise
    return xlds_end(L, o);
}

struct XLdsVfi { unsigned Vsh, Pish, ash, redsh, ctl; size_t bytes; };
XLDS_HD inline XLdsVfi xlds_vfi(int n_e, int n_a) {
    XLdsCursor o = {0, 0}; XLdsVfi L;
    L.Vsh = xlds_take(o, (size_t)n_e * 64, 8);               // [n_e][64]
    L.Pish = xlds_take(o, (size_t)n_e * n_e, 8);             // [n_e*n_e]
    L.ash = xlds_take(o, n_a, 8);                            // [n_a]
    L.redsh = xlds_take(o, 16, 8);                           // [16] per-wave max; [15]: the group's
    return xlds_end(L, o);
}

struct XLdsStat { unsigned tile, redsh, ctl; size_t bytes; };
XLDS_HD inline XLdsStat xlds_stat(int n_e) {
    XLdsCursor o = {0, 0}; XLdsStat L;
    L.tile = xlds_take(o, (size_t)n_e * 64, 8);              // [n_e][64]
    L.redsh = xlds_take(o, 16, 8);                           // [16] per-wave max
    return xlds_end(L, o);
}

struct XLdsTanBack { unsigned tile, rhosh, pxsh, dxsh, srcsh, ctl; size_t bytes; };
XLDS_HD inline XLdsTanBack xlds_tan_back(int n_e, int P, int D) {      // the group's input tangents of every period
    XLdsCursor o = {0, 0}; XLdsTanBack L;
    L.tile = xlds_take(o, (size_t)xtile_sl(D) * n_e * 64, 8);     // [n_e][64][SL]
    L.rhosh = xlds_take(o, (size_t)P + 1, 8);                // [P] + one pad
    L.pxsh = xlds_take(o, 3 * (size_t)P + 1, 8);             // [P][3]: 1 + r_t, w_t, tr_t (record diet) + one pad
    L.dxsh = xlds_take(o, 3 * (size_t)P * D, 8);             // [P][3][D]: this group's dr, dw, dtr (a cold uniform load per period otherwise)
    L.srcsh = xlds_take(o, P, 4);                            // [P] int: this member's source ranges
    return xlds_end(L, o);
}

// (ash is padded to a PAIR: xsh and dxsh are then on multiples of 16 the compiler can see, and it reads them 16 bytes at a time. The size
// the host has always asked for counts n_a + 1: at an even n_a the element the pair does not need stands behind dxsh)
struct XLdsDualBack { unsigned tile, ash, xsh, dxsh, ctl; size_t bytes; };
XLDS_HD inline XLdsDualBack xlds_dual_back(int n_e, int n_a, int P, int D) {
    XLdsCursor o = {0, 0}; XLdsDualBack L;
    L.tile = xlds_take(o, (size_t)xslots(D + 1).SL * n_e * 64, 8);      // [n_e][64][SL]: slots 0..D-1 the partials of V, slot D the value
    L.ash = xlds_take(o, ((size_t)n_a + 1) & ~(size_t)1, 8);      // [n_a], padded to a pair
    L.xsh = xlds_take(o, 4 * (size_t)P, 8);                  // [P][4]: r_t, w_t, tr_t, rho_t
    L.dxsh = xlds_take(o, 3 * (size_t)P * D + ((n_a + 1) & 1), 8);      // [P][3][D]: this group's dr, dw, dtr (+ one pad at an even n_a)
    return xlds_end(L, o);
}

// (aggsh stands in front of Pish: behind the tile it is on a multiple of 16 at every n_e, and the pad behind Pish can be unconditional)
struct XLdsFwd { unsigned tile, aggsh, Pish, closh, srcsh, ctl; size_t bytes; };
XLDS_HD inline XLdsFwd xlds_fwd(int n_e, int P, int D, bool val) {      // with the kernel's own NSL and NAP
    const int NSL = D + (val ? 1 : 0), NAP = 2 * NSL;
    XLdsCursor o = {0, 0}; XLdsFwd L;
    L.tile = xlds_take(o, (size_t)xslots(NSL).SL * n_e * 64, 8);        // [n_e][64][SL]
    L.aggsh = xlds_take(o, (size_t)n_e * 64 * NAP, 8);       // [n_e][64][NAP]: the aggregate's terms of a period, per lane
    L.Pish = xlds_take(o, (size_t)n_e * n_e + 1, 8);         // [n_e*n_e] (read when the mixing's coefficients are not in registers) + one pad
    L.closh = xlds_take(o, (size_t)P * n_e, 4);              // [P][n_e] int: the clamped-prefix lengths (a cold uniform load per period otherwise)
    L.srcsh = xlds_take(o, P, 4);                            // [P] int
    return xlds_end(L, o);
}

// The Dual pass's forward sweep that reads the packed lottery record (k_xfwd<D, true, MAXT, true>): xlds_fwd's pieces where xlds_fwd puts them, then
// the inverse-gap table in front of ctl. srcsh ends on a multiple of 4: the table starts on the next multiple of 16.
struct XLdsFwdLq { unsigned tile, aggsh, Pish, closh, srcsh, iga, ctl; size_t bytes; };
XLDS_HD inline XLdsFwdLq xlds_fwd_lq(int n_e, int n_a, int P, int D) {
    const XLdsFwd F = xlds_fwd(n_e, P, D, true);
    XLdsFwdLq L;
    L.tile = F.tile; L.aggsh = F.aggsh; L.Pish = F.Pish; L.closh = F.closh; L.srcsh = F.srcsh;
    XLdsCursor o = {F.ctl, F.bytes - XCTL_BYTES};
    xlds_take(o, (16 - F.ctl % 16) % 16, 1);                 // pad
    L.iga = xlds_take(o, n_a, 8);                            // [n_a]: 1 / (a[l+1] - a[l]), the last entry 0 (k_iga_build)
    return xlds_end(L, o);
}

// ... and its tile SLOT-MAJOR (HANK_XFWD_TILE_SOA): [column][slot][lane] in doubles, the NSL = D + 1 live slots only — no pad slot,
// NSL / SL of the piece's bytes (5/6 at D = 4), the piece and everything behind it where xlds_fwd puts them. Consecutive target rows
// of one slot are consecutive doubles: the source walk's 8-byte adds and the mixing's 8-byte reads meet no bank twice in 16 lanes.
constexpr int XTILE_SOA_SLOT = 64;                                         // doubles from a slot to the next of the same column and lane
XLDS_HD inline unsigned xtile_soa_at(int NSL, int col, int slot, int lane) {      // an entry's offset in the tile piece (bytes)
    return (unsigned)(((col * NSL + slot) * XTILE_SOA_SLOT + lane) * 8);
}
XLDS_HD inline size_t xtile_soa_bytes(int n_e, int NSL) { return (size_t)n_e * NSL * XTILE_SOA_SLOT * 8; }      // <= the tile piece: NSL <= xslots(NSL).SL

}  // namespace hank
