// host_guide.h -- what dp_guide.hip (the k-mer distances on the device) and host_guide.cpp (cleaning, the distance formula,
// UPGMA) share.  The definition is in include/pagan_host.h.
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

} // namespace pagan

#endif
