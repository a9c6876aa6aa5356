/* mask_oracle.c -- the CPU statement of the region mask (klt_hip_set_mask,
 * include/klt_hip.h) for the tests.  The oracle itself is included as it
 * stands, so that the shim calls its own eigen_points / quicksort / track_one /
 * frame_pyramid; three functions are added:
 *   orc_select_mask, orc_replace_mask: select_impl with every masked pixel
 *     marked in min_distance's `taken` before the first point is visited;
 *   orc_track_mask: track_impl's loop with the mask test after the border test.
 * mask: one byte per pixel, H rows `pitch` >= W bytes apart, zero = masked;
 * NULL: no mask (the oracle's own results). */
#include "../../oracle/klt_oracle.c"

#define ORC_MASKED (-7)

/* min_distance (_enforceMinimumDistance + _fillFeaturemap) with the pre-marked map */
static void min_distance_mask(const int *pts, int npts, int nfeat, float *fx, float *fy, int *fval,
                              int W, int H, int mindist, int min_eig, int overwrite_all,
                              const uint8_t *mask, long pitch)
{
  unsigned char *taken = (unsigned char *)calloc((size_t)W * H, 1);
  int k = 0, p = 0, x, y, u, v, val;
  if (min_eig < 1) min_eig = 1;
  mindist--;

  if (mask)
    for (y = 0; y < H; y++)
      for (x = 0; x < W; x++)
        if (mask[(size_t)y * pitch + x] == 0) taken[(size_t)y * W + x] = 1;

  if (!overwrite_all)
    for (k = 0; k < nfeat; k++)
      if (fval[k] >= 0) {
        int cx = (int)fx[k], cy = (int)fy[k];
        for (v = cy - mindist; v <= cy + mindist; v++)
          for (u = cx - mindist; u <= cx + mindist; u++)
            if (u >= 0 && u < W && v >= 0 && v < H) taken[(size_t)v * W + u] = 1;
      }

  k = 0;
  for (;;) {
    if (p >= npts) {
      for (; k < nfeat; k++)
        if (overwrite_all || fval[k] < 0) {
          fx[k] = -1;
          fy[k] = -1;
          fval[k] = -1; /* KLT_NOT_FOUND */
        }
      break;
    }
    x = pts[3 * p];
    y = pts[3 * p + 1];
    val = pts[3 * p + 2];
    p++;
    while (!overwrite_all && k < nfeat && fval[k] >= 0) k++;
    if (k >= nfeat) break;
    if (!taken[(size_t)y * W + x] && val >= min_eig) {
      fx[k] = (float)x;
      fy[k] = (float)y;
      fval[k] = val;
      k++;
      for (v = y - mindist; v <= y + mindist; v++)
        for (u = x - mindist; u <= x + mindist; u++)
          if (u >= 0 && u < W && v >= 0 && v < H) taken[(size_t)v * W + u] = 1;
    }
  }
  free(taken);
}

/* select_impl with min_distance_mask: the point list and its quicksort are
 * those of the whole map */
static void select_impl_mask(orc_tracker *t, const uint8_t *img, int W, int H, int nfeat, float *fx,
                             float *fy, int *fval, int replacing, const uint8_t *mask, long pitch)
{
  orc_params *P = &t->P;
  const float *gx, *gy;
  float *own_img = NULL, *own_gx = NULL, *own_gy = NULL;
  int *pts, npts;
  size_t n = (size_t)W * H;

  if (replacing && P->sequentialMode && t->last) {
    gx = t->last->gx[0];
    gy = t->last->gy[0];
  } else {
    float *f = (float *)malloc(sizeof(float) * n);
    size_t i;
    own_img = (float *)malloc(sizeof(float) * n);
    own_gx = (float *)malloc(sizeof(float) * n);
    own_gy = (float *)malloc(sizeof(float) * n);
    for (i = 0; i < n; i++) f[i] = (float)img[i];
    if (P->smoothBeforeSelecting)
      smooth(f, W, H, smooth_sigma(P), own_img);
    else
      memcpy(own_img, f, sizeof(float) * n);
    free(f);
    gradients(own_img, W, H, P->grad_sigma, own_gx, own_gy);
    gx = own_gx;
    gy = own_gy;
  }
  pts = (int *)malloc(sizeof(int) * 3 * (n ? n : 1));
  npts = orc_eigen_points(P, gx, gy, W, H, pts);
  orc_quicksort(pts, npts);
  if (P->mindist < 0) P->mindist = 0;
  min_distance_mask(pts, npts, nfeat, fx, fy, fval, W, H, P->mindist, P->min_eigenvalue, !replacing,
                    mask, pitch);
  free(pts);
  free(own_img);
  free(own_gx);
  free(own_gy);
}

ORC_EXPORT void orc_select_mask(orc_tracker *t, const uint8_t *img, int W, int H, int nfeat,
                                float *fx, float *fy, int *fval, const uint8_t *mask, long pitch)
{
  fix_window(&t->P);
  select_impl_mask(t, img, W, H, nfeat, fx, fy, fval, 0, mask, pitch);
}

ORC_EXPORT void orc_replace_mask(orc_tracker *t, const uint8_t *img, int W, int H, int nfeat,
                                 float *fx, float *fy, int *fval, const uint8_t *mask, long pitch)
{
  int lost = 0, k;
  for (k = 0; k < nfeat; k++) lost += fval[k] < 0;
  fix_window(&t->P);
  if (lost > 0) select_impl_mask(t, img, W, H, nfeat, fx, fy, fval, 1, mask, pitch);
}

/* orc_track with the tracking rule.  pre (optional, nfeat ints): the status a
 * feature tracked by this call had before the mask test (what orc_track gives
 * it); prex / prey (optional): the position the mask test reads, (-1, -1)
 * where it does not apply (OOB, SMALL_DET).  Slots lost on entry are left
 * alone in all three. */
ORC_EXPORT void orc_track_mask(orc_tracker *t, const uint8_t *img1, const uint8_t *img2, int W,
                               int H, int nfeat, float *fx, float *fy, int *fval,
                               const uint8_t *mask, long pitch, int *pre, float *prex, float *prey)
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
    float xl, yl, xo, yo;
    int val = TRACKED, oob;
    if (fval[k] < 0) continue;
    xl = fx[k];
    yl = fy[k];
    for (r = P->nPyramidLevels - 1; r >= 0; r--) {
      xl /= ss;
      yl /= ss;
    }
    xo = xl;
    yo = yl;
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
    oob = val == OOB || xo < P->borderx || xo > W - 1 - P->borderx || yo < P->bordery ||
          yo > H - 1 - P->bordery;
    if (pre) pre[k] = oob ? OOB : val;
    if (prex) prex[k] = (oob || val == SMALL_DET) ? -1.0f : xo;
    if (prey) prey[k] = (oob || val == SMALL_DET) ? -1.0f : yo;
    if (oob) {
      fx[k] = -1.0f;
      fy[k] = -1.0f;
      fval[k] = OOB;
    } else if (mask && val != SMALL_DET && xo >= 0.0f && yo >= 0.0f && xo < (float)W &&
               yo < (float)H && mask[(size_t)(int)yo * pitch + (int)xo] == 0) {
      /* a test of position, like the border's: every level ran, so (xo, yo) is a
         level-0 position whatever the residue or the iteration count says */
      fx[k] = -1.0f;
      fy[k] = -1.0f;
      fval[k] = ORC_MASKED;
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
