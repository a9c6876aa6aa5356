/* frame_prior_oracle.c -- the CPU statement of the frame prior (DESIGN
 * section 4, "The frame prior") for the tests: the oracle's KLTTrackFeatures
 * loop with image 2's start taken from a caller-supplied 3x3 matrix in place
 * of xo = xl.  The oracle itself is included as it stands, so that the shim
 * calls its own track_one / frame_pyramid; one function is added.
 *
 * A row m0..m8 is a row-major 3x3 matrix that takes level-0 pixel coordinates
 * of image 1 to level-0 pixel coordinates of image 2.  One frame img1 -> img2
 * of a feature at (x, y) with val >= 0:
 *   1. with each operation rounded to float, in this order, no contraction:
 *        w  = (m6*x + m7*y) + m8
 *        gx = ((m0*x + m1*y) + m2) / w
 *        gy = ((m3*x + m4*y) + m5) / w          (IEEE-correct divisions);
 *   2. (gx, gy) goes through the divisions by the subsampling as (x, y) does
 *      and gives image 2's start; image 1's position is unchanged;
 *   3. at the coarsest level, after the first multiplication by the
 *      subsampling, a start whose window is not inside that level (the
 *      tracker's own bounds test; NaN and +-inf are not inside, which covers
 *      w == 0) is replaced by image 1's position there;
 *   4. everything else is KLTTrackFeatures as it stands; a slot with val > 0
 *      is tracked under the prior like any other, and there is no state.
 * Rules 2 and 3 are the motion prior's (klt_hip_set_predict, klt_hip.h).  The
 * identity row gives exactly orc_track: (1*x + 0*y) + 0 == x and x / 1 == x. */
#include "../../oracle/klt_oracle.c"

/* the tracker's bounds test (window_out) written as an inside test, so that a
 * NaN is not inside */
static int window_in(float x, float y, int hw, int hh, int nc, int nr)
{
  const float eps1 = 1.001f;
  return x - hw >= 0.0f && nc - (x + hw) >= eps1 && y - hh >= 0.0f && nr - (y + hh) >= eps1;
}

/* orc_track with the frame's row m0..m8: rules 1-4 above */
ORC_EXPORT void orc_track_frame_prior(orc_tracker *t, const uint8_t *img1, const uint8_t *img2,
                                      int W, int H, int nfeat, float *fx, float *fy, int *fval,
                                      const float *row)
{
  orc_params *P = &t->P;
  orc_pyr *p1, *p2;
  const float ss = (float)P->subsampling;
  int k, r;

  fix_window(P);
  if (P->sequentialMode && t->last) {
    p1 = t->last;
    if (p1->w[0] != W || p1->h[0] != H) {
      fprintf(stderr, "orc: image size changed in sequential mode\n");
      abort();
    }
  } else {
    p1 = frame_pyramid(P, img1, W, H);
  }
  p2 = frame_pyramid(P, img2, W, H);

  for (k = 0; k < nfeat; k++) {
    const float x0 = fx[k], y0 = fy[k];
    float xl, yl, xo, yo, a, b, w;
    int val = TRACKED;
    if (fval[k] < 0) continue;
    xl = x0;
    yl = y0;
    /* rule 1: one rounding per operation (built without contraction) */
    a = row[6] * x0;
    b = row[7] * y0;
    w = a + b;
    w = w + row[8];
    a = row[0] * x0;
    b = row[1] * y0;
    xo = a + b;
    xo = xo + row[2];
    xo = xo / w;
    a = row[3] * x0;
    b = row[4] * y0;
    yo = a + b;
    yo = yo + row[5];
    yo = yo / w;
    for (r = P->nPyramidLevels - 1; r >= 0; r--) { /* rule 2 */
      xl /= ss;
      yl /= ss;
      xo /= ss;
      yo /= ss;
    }
    for (r = P->nPyramidLevels - 1; r >= 0; r--) {
      orc_level A = {p1->img[r], p1->gx[r], p1->gy[r], p1->w[r], p1->h[r]};
      orc_level B = {p2->img[r], p2->gx[r], p2->gy[r], p2->w[r], p2->h[r]};
      xl *= ss;
      yl *= ss;
      xo *= ss;
      yo *= ss;
      if (r == P->nPyramidLevels - 1 && /* rule 3 */
          !window_in(xo, yo, P->window_width / 2, P->window_height / 2, B.w, B.h)) {
        xo = xl;
        yo = yl;
      }
      val = track_one(xl, yl, &xo, &yo, &A, &B, P);
      if (val == SMALL_DET || val == OOB) break;
    }
    if (val == OOB || xo < P->borderx || xo > W - 1 - P->borderx || yo < P->bordery ||
        yo > H - 1 - P->bordery) {
      fx[k] = -1.0f;
      fy[k] = -1.0f;
      fval[k] = OOB;
    } else if (val != TRACKED) {
      fx[k] = -1.0f;
      fy[k] = -1.0f;
      fval[k] = val;
    } else {
      fx[k] = xo;
      fy[k] = yo;
      fval[k] = TRACKED;
    }
  }

  if (P->sequentialMode)
    t->last = p2;
  else
    pyr_free(p2);
  pyr_free(p1);
}
