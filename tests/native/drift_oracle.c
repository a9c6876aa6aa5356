/* drift_oracle.c -- the definition and the CPU statement of the drift check
 * ("The drift check"): the oracle's KLTTrackFeatures loop,
 * then for a feature it leaves KLT_TRACKED the first-window template's store
 * or test.  The oracle itself is included as it stands, so that the shim calls
 * its own track_one / frame_pyramid / bilerp; one function is added.
 *
 * Setting: max_residue, finite and >= 0 or +inf; max_age >= 0.  State per
 * slot: age (0: no template; k >= 1: a template that has been through k - 1
 * tests) and tmpl, 49 floats row-major in window order, meaningful while
 * age > 0.  One frame img1 -> img2 for a feature at (x, y) with status val:
 *   1. val != 0 on entry sets age = 0; val < 0 is lost and not tracked, val > 0
 *      (fresh from selection or replacement) is tracked;
 *   2. the translation step is KLTTrackFeatures as it stands; a feature that
 *      does not end it KLT_TRACKED inside the border gets age = 0 and is
 *      otherwise the plain tracker's result;
 *   3. one that ends it KLT_TRACKED with age == 0 stores tmpl[q] =
 *      interpolate(x1 + i, y1 + j, img1 level 0), (x1, y1) the level-0 position
 *      the Newton loop used for image 1, and gets age = 1: no test;
 *   4. one that ends it KLT_TRACKED with age > 0 is tested: e = (sum_q |tmpl[q] -
 *      interpolate(xo + i, yo + j, img2 level 0)|) / 49, a sequential float sum
 *      from +0 in window order, each |a - b| rounded to float, one IEEE division
 *      (the residue's own arithmetic).  e > max_residue loses it: x = y = -1,
 *      val = -8 (DRIFTED), age = 0.  Otherwise age += 1, and if max_age > 0 and
 *      age > max_age, age = 0: the next tracked frame stores a new template;
 *   5. err (optional) holds e per feature, -1 where no test ran.
 * With max_residue = +inf every list is the plain tracker's, byte for byte. */
#include "../../oracle/klt_oracle.c"

#define ORC_DRIFTED (-8)

/* orc_track with the per-slot state (tmpl: 49 floats per slot in window order,
 * age) and the setting (max_residue, max_age): rules 1-5 above.  err
 * (optional, nfeat floats): e where a test ran, -1 elsewhere. */
ORC_EXPORT void orc_track_drift(orc_tracker *t, const uint8_t *img1, const uint8_t *img2, int W,
                                int H, int nfeat, float *fx, float *fy, int *fval,
                                float max_residue, int max_age, float *tmpl, int *age, float *err)
{
  orc_params *P = &t->P;
  orc_pyr *p1, *p2;
  const float ss = (float)P->subsampling;
  int k, r, i, j, q;

  fix_window(P);
  if (P->window_width != 7 || P->window_height != 7 || P->lighting_insensitive) {
    fprintf(stderr, "orc: the drift check is stated for the 7x7 window without gain/bias\n");
    abort();
  }
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
    float xl, yl, xo, yo, *tm = tmpl + (size_t)49 * k;
    int val = TRACKED;
    if (err) err[k] = -1.0f;
    if (fval[k] != 0) age[k] = 0; /* rule 1 */
    if (fval[k] < 0) continue;
    xl = xo = fx[k];
    yl = yo = fy[k];
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
    if (fval[k] != TRACKED) { /* rule 2 */
      age[k] = 0;
      continue;
    }
    if (age[k] == 0) { /* rule 3: the window the residue pass read for image 1 */
      q = 0;
      for (j = -3; j <= 3; j++)
        for (i = -3; i <= 3; i++, q++) tm[q] = bilerp(xl + i, yl + j, p1->img[0], p1->w[0]);
      age[k] = 1;
      continue;
    }
    { /* rule 4 */
      float s = 0.0f, e;
      q = 0;
      for (j = -3; j <= 3; j++)
        for (i = -3; i <= 3; i++, q++) {
          const float d = tm[q] - bilerp(xo + i, yo + j, p2->img[0], p2->w[0]);
          s += (float)fabs(d);
        }
      e = s / 49;
      if (err) err[k] = e;
      if (e > max_residue) {
        fx[k] = -1.0f;
        fy[k] = -1.0f;
        fval[k] = ORC_DRIFTED;
        age[k] = 0;
      } else {
        age[k] += 1;
        if (max_age > 0 && age[k] > max_age) age[k] = 0;
      }
    }
  }

  if (P->sequentialMode)
    t->last = p2;
  else
    pyr_free(p2);
  pyr_free(p1);
}
