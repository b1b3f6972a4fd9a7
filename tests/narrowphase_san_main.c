/* test tool (tests/test_narrowphase.py): a stand-alone program around the checker's per-pair entry osim_narrowphase, so that the entry
 * and everything below it (oracle/fsim_oracle.c) can run under AddressSanitizer + UndefinedBehaviorSanitizer as an ordinary executable.
 * in:  int32 ncase, t1, t2, nvert; double verts[3 * nvert]; per case 31 doubles: p1[3] R1[9] s1[3] p2[3] R2[9] s2[3] margin
 * out: per case int32 count, double contacts[16][7] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../oracle/fsim_oracle.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t hd[4];
  if (fread(hd, sizeof hd, 1, in) != 1 || hd[0] < 0 || hd[3] < 0) return 3;
  const int n = hd[0], t1 = hd[1], t2 = hd[2], nvert = hd[3];
  double *verts = (double *)malloc(sizeof(double) * 3 * (size_t)(nvert > 0 ? nvert : 1));
  if (!verts || fread(verts, sizeof(double) * 3, (size_t)nvert, in) != (size_t)nvert) return 3;
  for (int i = 0; i < n; i++) {
    double c[31], con[16][7];
    if (fread(c, sizeof c, 1, in) != 1) return 3;
    memset(con, 0, sizeof con);
    int32_t cnt = osim_narrowphase(t1, c, c + 3, c + 12, t1 == 7 ? verts : NULL, t1 == 7 ? nvert : 0,
                                   t2, c + 15, c + 18, c + 27, t2 == 7 ? verts : NULL, t2 == 7 ? nvert : 0, c[30], con);
    fwrite(&cnt, sizeof cnt, 1, out);
    fwrite(con, sizeof con, 1, out);
  }
  free(verts);
  fclose(in);
  return fclose(out) ? 4 : 0;
}
