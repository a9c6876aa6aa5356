/* predict_oracle.c -- the CPU statement of the motion prior
 * (klt_hip_set_predict, include/klt_hip.h) for the tests: the oracle's
 * KLTTrackFeatures loop with a predicted start for image 2 in place of
 * xo = xl.  The oracle itself is included as it stands, so that the shim calls
 * its own track_one / frame_pyramid; one function is added. */
#include "../../oracle/klt_oracle.c"

/* the tracker's bounds test (window_out) written as an inside test, so that a
 * NaN is not inside */
static int window_in(float x, float y, int hw, int hh, int nc, int nr)
{
  const float eps1 = 1.001f;
  return x - hw >= 0.0f && nc - (x + hw) >= eps1 && y - hh >= 0.0f && nr - (y + hh) >= eps1;
}

/* orc_track with the per-feature state (vx, vy): rules 1-5 of klt_hip.h */
ORC_EXPORT void orc_track_predict(orc_tracker *t, const uint8_t *img1, const uint8_t *img2, int W,
                                  int H, int nfeat, float *fx, float *fy, int *fval, float *vx,
                                  float *vy)
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
    float xl, yl, xo, yo;
    int val = TRACKED;
    if (fval[k] != 0) { /* rule 1 */
      vx[k] = 0.0f;
      vy[k] = 0.0f;
    }
    if (fval[k] < 0) continue;
    xl = x0;
    yl = y0;
    xo = x0 + vx[k]; /* rule 2 */
    yo = y0 + vy[k];
    for (r = P->nPyramidLevels - 1; r >= 0; r--) {
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
    if (fval[k] == TRACKED) { /* rule 5 */
      vx[k] = xo - x0;
      vy[k] = yo - y0;
    } else {
      vx[k] = 0.0f;
      vy[k] = 0.0f;
    }
  }

  if (P->sequentialMode)
    t->last = p2;
  else
    pyr_free(p2);
  pyr_free(p1);
}
