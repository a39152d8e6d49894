// TEST INFRASTRUCTURE ONLY: stand-in for the third-party <pdqsort.h> named by the reference's collision/capt.hh and
// collision/filter.hh (one call each to pdqsort_branchless(begin, end, comp)).  An unstable sort leaves only the order
// of equal keys open; the two variants below fix that order in opposite ways, so a result that is byte-identical under
// both does not depend on it (tools/make_cloud_golden.py: the tie-order certificate).
#pragma once
#include <algorithm>
#include <chrono>    // capt.hh names std::chrono and std::cerr without including them
#include <iostream>

template <class It, class Comp>
inline void pdqsort_branchless(It begin, It end, Comp comp)
{
#ifdef REF_TIES_REVERSED
    std::reverse(begin, end);
#endif
    std::stable_sort(begin, end, comp);
}

template <class It, class Comp>
inline void pdqsort(It begin, It end, Comp comp)
{
    pdqsort_branchless(begin, end, comp);
}
