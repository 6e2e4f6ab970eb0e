// letter_codes_check.cpp -- stand-alone host program around the two sequence encodings of the library (ractip_amd/csrc/constraint_prepass.cpp:
// nuc_code for the CONTRAfold model, vienna_code for the Vienna model).  No GPU, no HIP:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc \
//       tools/letter_codes_check.cpp ractip_amd/csrc/constraint_prepass.cpp -o letter_codes_check
//   ./letter_codes_check
//
// Prints one line "byte nuc_code vienna_code" per byte value 0..255 (tests/test_unknown_letters_cpu.py compares them with the
// encodings of oracle/cf_oracle.c and oracle/vienna_oracle.c), and checks here that the letter the helper context writes back for a
// Vienna code ("NACGU"[code], fallbacks.hip) encodes to the same code again; exit status 0 iff it does.
#include <cstdio>

#include "constraint_prepass.h"

int main()
{
    int bad = 0;
    for (int b = 0; b < 256; b++) {
        const int nc = rh::host::nuc_code((char)b), vc = rh::host::vienna_code((char)b);
        std::printf("%d %d %d\n", b, nc, vc);
        if (nc < 0 || nc > 4 || vc < 0 || vc > 4) bad++;
        if (rh::host::vienna_code("NACGU"[vc]) != vc) bad++;
    }
    std::printf("%d failures\n", bad);
    return bad ? 1 : 0;
}
