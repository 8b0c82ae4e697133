// w2b_evalclasses.h -- launchers of w2b_kernels_evalclasses.hip for the host side of w2b_eval_classes (w2b_eval.cpp;
// include/word2bits_eval.h, "word classes").  B = the packed rows as 64-bit words, [words][bitlevel * ceil(dim / 64)];
// K = n_classes; every class id in `cl` must lie in [0, K).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// classes rounded up to whole pairs of 32-class tiles: the length of wq, and 32 times the number of `live` words
long long w2b_cls_class_slots(int K);
// bytes of the centroid operands in fragment order (the operand kernel writes every byte of them)
size_t w2b_cls_operand_bytes(int dim, int K);
// The sums pass of one class array: a counting sort of the rows by class (hist [K] -> start [K + 1], cursor [K], order
// [words]; counts [K] = the members), the pooled integer sums T [K][dim], N [K] = sum_a T[a]^2 and X = the centroid
// operands.  The launcher zeroes what it needs zeroed itself.
hipError_t w2b_launch_cls_sums(const uint64_t *B, int words, int dim, int bitlevel, int K, const int *cl, int *hist, int *start,
                               int *cursor, int *order, int *T, long long *counts, long long *N, void *X, hipStream_t s);
// The assign scan: cl_new[c] = the live class with the largest d = S * wq (ties to the lowest class; 0 when no class is
// live), score[c] = that d (+0 when none), *moved += the rows with cl_new[c] != cl[c].  wq = [w2b_cls_class_slots(K)], live
// = one bit per class in 32-bit words, clear for a dead class and for the slots past K.
hipError_t w2b_launch_cls_assign(const uint64_t *B, int words, int dim, int bitlevel, int K, const void *X, const float *wq,
                                 const uint32_t *live, const int *cl, int *cl_new, float *score, unsigned long long *moved,
                                 hipStream_t s);
