// host_nj.h -- what dp_nj.hip (the join loop of neighbour joining on the device) and host_nj.cpp (the checks, the byte count, the
// rooting and the printing) share.  The definition is in include/pagan_host.h, "neighbour joining".
#ifndef PAGAN_HOST_NJ_H
#define PAGAN_HOST_NJ_H

#include <cstddef>
#include <cstdint>

namespace pagan {

// a row's best pair: Q, the pair's ids (ia < ib) and the slots of the row and of the column (sa < sb)
struct NjRowBest { double q; int32_t ia, ib, sa, sb; };
// what pick hands to merge: d(i, j) and the slots of i and j (the ids' order, not the slots')
struct NjPick { double dij; int32_t si, sj; };
// the log: a record a join, then the star
struct NjRecord { int32_t i, j; double len_i, len_j; };
struct NjStar { int32_t ids[3], pad; double len[3]; };
static_assert(sizeof(NjRowBest) == 24 && sizeof(NjPick) == 16 && sizeof(NjRecord) == 24 && sizeof(NjStar) == 40, "device records");

// the device buffers of one pagan_nj_joins call, carved from one allocation (n >= 3)
struct NjLayout {
    size_t matrix, R, id, best, cur, log, total;     // log: n - 3 records, then the star
    explicit NjLayout(int64_t n);
};

// PAGAN_OK, or PAGAN_E_ARG: n outside 2 .. PAGAN_NJ_MAX_SEQS, no matrix, an entry above the diagonal that is not finite or < 0
int nj_check_input(int32_t n, const double *dist);

} // namespace pagan

#endif
