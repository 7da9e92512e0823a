// Host-side check of the position logic of rafft_amd/csrc/rafft_moves.h, built host-only with hipcc by tests/test_descend_host.py:
// for every (sequence, row) the moves that enclosing_pair and next_partner yield over all positions x - the removal of the pair
// whose 5' end x is, the additions with x as 5' end - against a brute force written here (every (i, j) with j - i > 3, both
// unpaired, a canonical pair of letters, crossing no pair; every pair as a removal) and against the list the test passes in.  Each
// row twice: next_partner up to the 3' end of the enclosing pair (descend, kinfold) and up to L (barriers).  apply_move is checked
// on the way: every move applied and taken back leaves the table as it was.  dE is device code and not checked here.
// usage: moves_check [SEQ ROW MOVES]...   MOVES = "i-j-r,i-j-a,..." (r: removal, a: addition; ascending (i, j)).  Test infrastructure.
#include <cstdio>
#include <cstdlib>
#include <string>
#include "../../rafft_amd/csrc/rafft_moves.h"
#include "../../rafft_amd/csrc/rafft_hostpure.h"

static int fails = 0;

static std::string item(int i, int j, bool rem) { return std::to_string(i) + "-" + std::to_string(j) + (rem ? "-r," : "-a,"); }

static bool letters_pair(char a, char b)
{
    const std::string p{a, b};
    return p == "AU" || p == "UA" || p == "GC" || p == "CG" || p == "GU" || p == "UG";
}

static void check_case(const char *seq, const char *row, const char *want)
{
    const int L = (int)strlen(seq);
    std::vector<uint8_t> S((size_t)L + 16, 0);
    for (int x = 0; x < L; x++) S[x] = (uint8_t)(kBaseCode[(unsigned char)seq[x]] & 7);
    std::vector<int16_t> pt;
    if ((int)strlen(row) != L || descend_parse_row(S.data(), L, row, pt)) { fails++; fprintf(stderr, "FAIL %s %s: not a valid row\n", seq, row); return; }
    std::string brute;
    for (int i = 0; i < L; i++) {
        if (pt[i] > i) brute += item(i, pt[i], true);
        for (int j = i + 4; j < L && pt[i] < 0; j++) {
            if (pt[j] >= 0 || !letters_pair(seq[i], seq[j])) continue;
            bool crossed = false;
            for (int p = 0; p < L; p++) crossed |= pt[p] > p && ((p < i && i < pt[p] && pt[p] < j) || (i < p && p < j && j < pt[p]));
            if (!crossed) brute += item(i, j, false);
        }
    }
    std::string given = want;
    if (!given.empty()) given += ",";
    for (int to_L = 0; to_L < 2; to_L++) {
        std::string got;
        const std::vector<int16_t> before = pt;
        for (int x = 0; x < L; x++) {
            const int y = pt[x];
            if (y >= 0 && y < x) continue;
            if (y > x) {
                got += item(x, y, true);
                apply_move(pt.data(), x, y, true, nullptr, 0);
                if (pt[x] != -1 || pt[y] != -1) { fails++; fprintf(stderr, "FAIL %s %s: apply_move, removal of %d-%d\n", seq, row, x, y); }
                apply_move(pt.data(), x, y, false, nullptr, 0);
                continue;
            }
            int ci, cj;
            enclosing_pair(pt.data(), x, L, ci, cj);
            if (ci >= 0 ? !(ci < x && x < cj && pt[ci] == cj) : cj != L) { fails++; fprintf(stderr, "FAIL %s %s: enclosing_pair(%d) = (%d, %d)\n", seq, row, x, ci, cj); }
            const int end = to_L ? L : cj;
            for (int j = next_partner(pt.data(), S.data(), x, x, end); j < end; j = next_partner(pt.data(), S.data(), x, j, end)) {
                got += item(x, j, false);
                int mv[2] = {0, 0};
                apply_move(pt.data(), x, j, false, mv, 0);
                if (pt[x] != j || pt[j] != x || mv[0] != x || mv[1] != j) { fails++; fprintf(stderr, "FAIL %s %s: apply_move, addition of %d-%d\n", seq, row, x, j); }
                apply_move(pt.data(), x, j, true, mv, 0);
                if (mv[0] != -x - 1 || mv[1] != -j - 1) { fails++; fprintf(stderr, "FAIL %s %s: apply_move, the reported removal of %d-%d\n", seq, row, x, j); }
            }
        }
        if (pt != before) { fails++; fprintf(stderr, "FAIL %s %s: the table after every move was taken back\n", seq, row); pt = before; }
        if (got != brute) { fails++; fprintf(stderr, "FAIL %s %s (end = %s): %s, brute force %s\n", seq, row, to_L ? "L" : "cj", got.c_str(), brute.c_str()); }
        if (got != given) { fails++; fprintf(stderr, "FAIL %s %s (end = %s): %s, expected %s\n", seq, row, to_L ? "L" : "cj", got.c_str(), given.c_str()); }
    }
}

int main(int argc, char **argv)
{
    if ((argc - 1) % 3) { fprintf(stderr, "usage: moves_check [SEQ ROW MOVES]...\n"); return 2; }
    for (int k = 1; k + 2 < argc; k += 3) check_case(argv[k], argv[k + 1], argv[k + 2]);
    printf("%d cases, %d failures\n", (argc - 1) / 3, fails);
    return fails ? 1 : 0;
}
