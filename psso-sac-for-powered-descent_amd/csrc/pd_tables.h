// pd_tables.h -- the host table builder of libpdenv.so (pd_tables.hip): everything a handle's
// step kernel reads that is computed once on the CPU.  Pure host numerics, no HIP runtime call:
// pd_create (pdenv.hip) builds a HostTables, uploads its arrays and points D at the copies; the
// builder also runs stand-alone under host sanitizers (tests/native/tables_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/pdenv.h"
#include "pd_step.h"

namespace pd {

// the thread-local message behind pd_last_error() (pdenv.hip)
pd_status set_error(pd_status s, const char* m);

template <typename R> struct Table {
    int logcap = 0;
    std::vector<unsigned long long> keys;
    std::vector<R> pay;
    int64_t entries = 0;
};

// The cell pieces of one table's interior grid (see "cell pieces" in pd_tables.hip)
struct CellPieces {
    std::vector<double> rec;          // [n][kCellStride]: exact cells at their cell index, then refined cells' pieces
    std::vector<uint8_t> cell_ok;     // [nm na] the exact cell's own piece is valid
    std::vector<int> sub_piece;       // [refined][S][S] piece of an exact sub-cell's key (-1 none)
    std::vector<int> bis_a, bis_b;    // per GridKeys bisector record: each trusted side's piece
    std::vector<uint32_t> fine;       // [nm S][na S] fine index (pd_step.h kFinePiece)
    double max_rel = 0, build_s = 0;
    int64_t pieces = 0, rejected = 0;
    std::vector<double> err;          // per piece: the binary64 check's error (INFINITY: unused slot)
    std::vector<double> scale;        // per piece: the largest sum |c_j phi_j| + |s| at its check points
    std::vector<int> cell_of;         // per piece: its grid cell
    // the fine index's inputs (kept for the binary32 variant)
    int nm = 0, na = 0;
    double a0 = 0, dm = 0, da = 0;
    std::vector<uint8_t> refined;
    std::vector<int> ridx;
    std::vector<int64_t> bs_of;
    // binary32 handles (ensure_f32): the records in floats (kCellStrideF), each checked in binary32
    // against its binary64 piece; validity, sub-cell pieces, bisector sides and fine index of
    // the pieces that pass
    bool have32 = false;
    std::vector<float> rec32;
    std::vector<uint8_t> cell_ok32;
    std::vector<int> sub_piece32, bis_a32, bis_b32;
    std::vector<uint32_t> fine32;
    double max_rel32 = 0;
    int64_t rejected32 = 0;
};

// What a handle's tables consist of, as the host computes them.  pd_create uploads every array
// in this order (tay, atm, per grid key / slot / sub_key / sub_slot / bis, then the two hash
// tables) and stores the device addresses in D.
template <typename R> struct HostTables {
    DevParams<R> D;                 // every field the host knows; the device pointers still null
    Table<R> cd, cl;                // hash tables of solved neighbourhoods (C_D, C_L)
    std::vector<R> tay;             // Taylor pieces of the clamped query lines (D.tay_off)
    std::vector<R> atm;             // atmosphere cells, D.atm_n of them (empty: the exact formulas)
    // the coarse atmosphere records of the 512-thread kernels' LDS image (D.atl_n cells, then the
    // boundary cells' upper pieces; empty: none), part of the uploaded StepStatic image
    std::vector<R> atl;
    struct Grid {                   // interior candidate grid of one table
        std::vector<unsigned long long> key, sub_key;
        std::vector<int> slot, sub_slot;
        std::vector<GridBisect> bis;
        const CellPieces* pieces = nullptr;   // process-wide cache entry (nullptr: PD_TABLES_NO_CELL_PIECES)
        int nm = 0, na = 0;
        double a0 = 0, a1 = 0;
    } grid[2];
};
// Instantiated for double and float.  PD_TABLES_VERBOSE prints the builders' statistics to stderr.
template <typename R> pd_status build_host_tables(const pd_params* p, const pd_config* c, HostTables<R>& H);

// observation layout (obs_write) of a (phase, rtd) pair
int obs_kind_of(int phase, int rtd);
uint64_t host_knn_key(const pd_aero_table& t, double M, double a);
void grid_geometry(int tb, int& nm, int& na, double& a0, double& a1);
const CellPieces& cell_pieces(const pd_aero_table& t, double a0, double a1, int nm, int na);
void ensure_f32(CellPieces& cp);
// (instantiated for double and float)
template <typename R> void build_atm_table(const pd_params* P, std::vector<R>& out, int& n_cells, double& max_rel);
// (instantiated for double: the coarse table exists for binary64 handles)
template <typename R>
void build_atm_lds_table(const pd_params* P, std::vector<R>& out, int& n_cells, int& n_rec, double& max_rel);

// The device's Horner evaluation of coefficients q[0..deg] (in R) at t, in R
template <typename R> R horner_host(const R* q, int deg, R t) {
    R f = q[deg];
    for (int k = deg - 1; k >= 0; --k) f = (R)std::fma((double)f, (double)t, (double)q[k]);
    return f;
}

}  // namespace pd
