// host_guide.h -- what dp_guide.hip (the k-mer distances on the device) and host_guide.cpp (cleaning, the distance formula,
// UPGMA) share, and what dp_alndist.hip (row pair counts of an alignment) takes from host_guide.cpp.  The definitions are in
// include/pagan_host.h.
#ifndef PAGAN_HOST_GUIDE_H
#define PAGAN_HOST_GUIDE_H

#include <cstdint>
#include <string>
#include <vector>

namespace pagan {

// One byte per cleaned letter: its code (0..3 / 0..19) or kGuideNoLetter for a letter that is kept but is no core letter.
constexpr unsigned char kGuideNoLetter = 0xFF;

struct GuideInput {
    int data_type = 0;                   // 1 DNA, 2 protein, 3 codon (0 resolved)
    int bits = 2;                        // per letter
    int max_k = 31;
    int64_t longest = 0;
    std::vector<uint32_t> off;           // [n + 1] positions of the sequences in `letters`
    std::vector<unsigned char> letters;  // codes of all cleaned letters, concatenated
};

// pagan_msa_create's cleaning and type guess, then the letters' codes.  PAGAN_OK, or PAGAN_E_ARG (a null string, a
// data_type outside 0..3, more than PAGAN_GUIDE_MAX_POSITIONS letters).
int guide_clean(int32_t n, const char *const *seqs, int32_t data_type, GuideInput *out);
// 0: names fine; PAGAN_E_ARG: a null or empty name, or one with any of "(),:;" or white space
int guide_check_names(int32_t n, const char *const *names);

// ---- guide tree from an alignment (csrc/dp_alndist.hip; include/pagan_host.h, "guide tree from an alignment") ----
// The rows' common length and data type (1, 2, 3; 0 resolved by the walk's guess over the rows without their gap characters).
// PAGAN_OK, or PAGAN_E_ARG: n outside 2 .. PAGAN_GUIDE_MAX_SEQS, a null row, a ragged set, L >= 2^31, a data_type outside 0..3.
int aln_check_rows(int32_t n, const char *const *rows, int32_t data_type, int64_t *columns, int *resolved_type);
// table[c]: the code of character c (0..3 / 0..19), or kGuideNoLetter
void aln_letter_table(int data_type, unsigned char table[256]);
// workgroups that share the words of one tile: enough to fill the chip when the tiles alone do not
int aln_col_splits(int64_t tiles, int64_t words);

// the device buffers of one pagan_aln_distances call, carved from one allocation
struct AlnLayout {
    int64_t rows_pad, tiles, words, words_pad, slices;   // (words_pad: whole split granules)
    int planes, splits;
    size_t bytes, table, packed, out, total;
    AlnLayout(int64_t n, int64_t columns, int planes_);
};

} // namespace pagan

#endif
