/*
 * Stand-in for <cblas.h>, written from the public CBLAS interface (netlib's C interface to the BLAS).
 *
 * TEST INFRASTRUCTURE ONLY.  flappie_matrix.c and layers.c of the reference include <cblas.h> for two
 * prototypes and the enumerators they pass; the decode path that oracle/Makefile's `flappieref`
 * builds never calls either function (flappie_ref_main.c defines both as abort()).
 */
#ifndef FLAPPIE_REF_CBLAS_H
#define FLAPPIE_REF_CBLAS_H

enum CBLAS_ORDER { CblasRowMajor = 101, CblasColMajor = 102 };
enum CBLAS_TRANSPOSE { CblasNoTrans = 111, CblasTrans = 112, CblasConjTrans = 113 };

void cblas_sgemv(const enum CBLAS_ORDER order, const enum CBLAS_TRANSPOSE trans, const int m, const int n,
                 const float alpha, const float* a, const int lda, const float* x, const int incx,
                 const float beta, float* y, const int incy);
void cblas_sgemm(const enum CBLAS_ORDER order, const enum CBLAS_TRANSPOSE transa, const enum CBLAS_TRANSPOSE transb,
                 const int m, const int n, const int k, const float alpha, const float* a, const int lda,
                 const float* b, const int ldb, const float beta, float* c, const int ldc);

#endif
