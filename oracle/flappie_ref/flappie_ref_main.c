/*
 * flappie_ref_main.c -- a driver around the UNMODIFIED decode path of the reference's flappie
 * (flappie/src/decode.c, util.c, flappie_matrix.c, layers.c), linked by oracle/Makefile's `flappieref`
 * into oracle/_ref/flappie_decode.out.
 *
 * TEST INFRASTRUCTURE ONLY.  Written from scratch: it calls only what decode.h / flappie_matrix.h
 * declare (make_flappie_matrix, free_flappie_matrix, transpost_crf_flipflop, decode_crf_flipflop,
 * change_positions, base_lookup), in the order of flappie.c:266-285.
 *
 *   flappie_decode.out transpost IN OUT
 *       IN:  float32[nblk][40] transition scores (flappie's `trans` matrix, one column per block)
 *       OUT: float32[nblk][40] log-posteriors, transpost_crf_flipflop(trans, true): the first 40
 *            floats of every column of `stride`
 *   flappie_decode.out basecall IN OUT
 *       IN:  float32[nblk][40] posterior matrix
 *       OUT: int32 nblk, int32 path[nblk+1], float32 score, int32 nch, int32 chpos[nch], char bases[nch]
 *            decode_crf_flipflop(post, false, path, qpath), change_positions(path, nblk, chpos),
 *            bases[i] = base_lookup[path[chpos[i]] % 4]
 * Qualities (qpath, phredf) are not written: the project produces none.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cblas.h>
#include "decode.h"
#include "flappie_matrix.h"

#define NTRANS 40
#define NBASE 4

/* named by flappie_matrix.c and layers.c, never reached from the decode path */
void cblas_sgemv(const enum CBLAS_ORDER order, const enum CBLAS_TRANSPOSE trans, const int m, const int n,
                 const float alpha, const float* a, const int lda, const float* x, const int incx,
                 const float beta, float* y, const int incy) {
  (void)order; (void)trans; (void)m; (void)n; (void)alpha; (void)a; (void)lda; (void)x; (void)incx; (void)beta; (void)y; (void)incy;
  abort();
}

void cblas_sgemm(const enum CBLAS_ORDER order, const enum CBLAS_TRANSPOSE transa, const enum CBLAS_TRANSPOSE transb,
                 const int m, const int n, const int k, const float alpha, const float* a, const int lda,
                 const float* b, const int ldb, const float beta, float* c, const int ldc) {
  (void)order; (void)transa; (void)transb; (void)m; (void)n; (void)k; (void)alpha; (void)a; (void)lda; (void)b; (void)ldb; (void)beta; (void)c; (void)ldc;
  abort();
}

static int fail(const char* what) {
  fprintf(stderr, "flappie_decode: %s\n", what);
  return 1;
}

/* whole file -> a 40 x nblk matrix (column = block), NULL on any error */
static flappie_matrix read_matrix(const char* name) {
  FILE* f = fopen(name, "rb");
  if (!f) return NULL;
  if (fseek(f, 0, SEEK_END) != 0) { fclose(f); return NULL; }
  const long nbytes = ftell(f);
  rewind(f);
  if (nbytes <= 0 || nbytes % (long)(NTRANS * sizeof(float)) != 0) { fclose(f); return NULL; }
  const size_t nblk = (size_t)nbytes / (NTRANS * sizeof(float));
  flappie_matrix m = make_flappie_matrix(NTRANS, nblk);
  if (!m) { fclose(f); return NULL; }
  for (size_t blk = 0; blk < nblk; ++blk) {
    if (fread(m->data.f + blk * m->stride, sizeof(float), NTRANS, f) != NTRANS) {
      fclose(f);
      free_flappie_matrix(m);
      return NULL;
    }
  }
  fclose(f);
  return m;
}

static int do_transpost(const_flappie_matrix trans, FILE* out) {
  flappie_matrix post = transpost_crf_flipflop(trans, true);
  if (!post) return fail("transpost_crf_flipflop returned NULL");
  int bad = 0;
  for (size_t blk = 0; blk < post->nc && !bad; ++blk)
    bad = fwrite(post->data.f + blk * post->stride, sizeof(float), NTRANS, out) != NTRANS;
  free_flappie_matrix(post);
  return bad ? fail("short write") : 0;
}

static int do_basecall(const_flappie_matrix post, FILE* out) {
  const size_t nblk = post->nc;
  int* path = calloc(nblk + 2, sizeof(int));          /* sizes of flappie.c:259-261 */
  int* chpos = calloc(nblk + 2, sizeof(int));
  float* qpath = calloc(nblk + 2, sizeof(float));
  if (!path || !chpos || !qpath) return fail("out of memory");
  const float score = decode_crf_flipflop(post, false, path, qpath);
  const size_t nch = change_positions(path, nblk, chpos);
  char* bases = calloc(nch + 1, sizeof(char));
  if (!bases) return fail("out of memory");
  for (size_t i = 0; i < nch; ++i) bases[i] = base_lookup[path[chpos[i]] % NBASE];
  const int32_t n32 = (int32_t)nblk, nch32 = (int32_t)nch;
  int bad = sizeof(int) != sizeof(int32_t);
  bad = bad || fwrite(&n32, sizeof n32, 1, out) != 1;
  bad = bad || fwrite(path, sizeof(int32_t), nblk + 1, out) != nblk + 1;
  bad = bad || fwrite(&score, sizeof score, 1, out) != 1;
  bad = bad || fwrite(&nch32, sizeof nch32, 1, out) != 1;
  bad = bad || fwrite(chpos, sizeof(int32_t), nch, out) != nch;
  bad = bad || fwrite(bases, 1, nch, out) != nch;
  free(bases);
  free(qpath);
  free(chpos);
  free(path);
  return bad ? fail("short write") : 0;
}

int main(int argc, char** argv) {
  if (argc != 4 || (strcmp(argv[1], "transpost") != 0 && strcmp(argv[1], "basecall") != 0))
    return fail("usage: flappie_decode.out transpost|basecall IN OUT");
  flappie_matrix in = read_matrix(argv[2]);
  if (!in) return fail("cannot read a float32[nblk][40] matrix of at least one block");
  FILE* out = fopen(argv[3], "wb");
  if (!out) { free_flappie_matrix(in); return fail("cannot open the output file"); }
  const int rc = strcmp(argv[1], "transpost") == 0 ? do_transpost(in, out) : do_basecall(in, out);
  free_flappie_matrix(in);
  if (fclose(out) != 0) return fail("short write");
  return rc;
}
