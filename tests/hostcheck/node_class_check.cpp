// Host-side reader of the expand classes (rafft_amd/csrc/rafft_kernels.h), built host-only with hipcc by tests/test_class_edges.py.
// Test infrastructure, not product code.  First line: the constants the classes are cut by.  Then, for every line
//   n span nbr merge_cls cls1_P cls1_br K sm_n4 sm_n5
// on standard input, one line with node_class(...) of it.
#include <cstdio>
#include "../../rafft_amd/csrc/rafft_kernels.h"

int main()
{
    printf("SM_SPAN %d CLS01_L %d CLS1_P %d CLS1_BR %d CLS2_P %d MAX_P %d MAX_BR %d BIG_BR %d LDS_SEQ %d\n",
           SM_SPAN, CLS01_L, CLS1_P, CLS1_BR, CLS2_P, MAX_P, MAX_BR, BIG_BR, LDS_SEQ);
    int n, span, nbr, merge, p1, br1, K, s4, s5;
    while (scanf("%d %d %d %d %d %d %d %d %d", &n, &span, &nbr, &merge, &p1, &br1, &K, &s4, &s5) == 9)
        printf("%d\n", node_class(n, span, nbr, merge, p1, br1, K, s4, s5));
    return 0;
}
