// Prints DeBERTa's bucket rule as the library computes it (kirag_amd/csrc/encoder_model.hpp: deberta_bucket), without a device (tests/test_deberta_host.py).
// argv: Bk M EXTRA.  stdout: one line "r p" for every column difference r in -(M - 1 + EXTRA) .. M - 1 + EXTRA.
#include "../../kirag_amd/csrc/encoder_model.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int Bk = atoi(argv[1]), M = atoi(argv[2]), extra = atoi(argv[3]);
    if (Bk < 2 || Bk % 2 || !(M - 1 > Bk / 2) || extra < 0) return 2;
    for (int r = -(M - 1 + extra); r <= M - 1 + extra; ++r) printf("%d %d\n", r, kr::model::deberta_bucket(r, Bk, M));
    return 0;
}
