// Prints the G / BT / AT tables of bsvd_amd/csrc/wino_forms.h (F(2,3) and F(6,3)) as hexadecimal doubles, one table per line:
//     F<M> <name> <rows> <cols> v v v ...
// tests/test_split_model_cpu.py compares them entry by entry with the tables tests/split_model.py restates, so the CPU model of the
// split arithmetic and the kernels cannot drift apart.  Plain g++, no HIP.
#include <cstdio>

#include "wino_forms.h"

template <int R, int C> static void dump(int m, const char *name, const double (&t)[R][C])
{
    std::printf("F%d %s %d %d", m, name, R, C);
    for (int r = 0; r < R; ++r)
        for (int c = 0; c < C; ++c) std::printf(" %a", t[r][c]);
    std::printf("\n");
}

template <int M> static void form()
{
    using W = bsvd::WinoForm<M>;
    dump(M, "G", W::G);
    dump(M, "BT", W::BT);
    dump(M, "AT", W::AT);
}

int main()
{
    form<2>();
    form<6>();
    return 0;
}
