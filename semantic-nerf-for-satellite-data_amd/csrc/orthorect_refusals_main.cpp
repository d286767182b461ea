// The refusal paths of snerf_orthorectify (orthorect.hip): see refusals_main.h.
#include "refusals_main.h"
#include "../../include/snerf_orthorect.h"

#include <climits>

// never dereferenced as device memory: every call is refused before a launch
static float dsm[12], rgbs[3 * 40], rgb_out[2 * 3 * 12];
static unsigned char labels[40], visible[2 * 12], label_out[2 * 12], state_out[2 * 12];
static long long sum[3 * 12];
static unsigned count[12], votes[5 * 12];
static double col_row[2 * 2 * 12];
static unsigned long long stats[4];
static SnerfRectImage images[SNERF_RECT_MAX_IMAGES + 1];
static SnerfDsmGrid grid = {1000.0, 2000.0, 0.5, 4, 3, 0, 0, 4, 3};
static const double LON0 = -1.4137166941154069;      // zone 17

struct Args {
  const float* dsm = ::dsm;
  const SnerfDsmGrid* grid = &::grid;
  double lon0 = LON0;
  int south = 0;
  const SnerfRectImage *host = images, *dev = images;
  int n_images = 2;
  const float* rgbs = ::rgbs;
  const unsigned char* labels = ::labels;
  long long n_rows = 40;
  int n_classes = 5;
  long long* sum = ::sum;
  unsigned* count = ::count;
  unsigned* votes = ::votes;
  unsigned long long* stats = ::stats;
};

static int call(const Args& a) {
  return snerf_orthorectify(a.dsm, a.grid, a.lon0, a.south, a.host, a.dev, a.n_images, a.rgbs, a.labels, a.n_rows, a.n_classes, visible,
                            a.sum, a.count, a.votes, col_row, rgb_out, label_out, state_out, a.stats, nullptr);
}

int main() {
  g_prefix = "snerf_orthorectify: ";
  what_width = 52;
  for (int k = 0; k <= SNERF_RECT_MAX_IMAGES; ++k) {
    SnerfRectImage& im = images[k];
    im.rpc.row_scale = im.rpc.col_scale = im.rpc.lat_scale = im.rpc.lon_scale = im.rpc.alt_scale = 1.0;
    im.row0 = 20 * (k & 1);
    im.w = 5;
    im.h = 4;
  }
  Args a;
  a = Args(); a.dsm = nullptr;    expect("null dsm", call(a), SNERF_ERR_NULL, "null");
  a = Args(); a.grid = nullptr;   expect("null grid", call(a), SNERF_ERR_NULL, "null");
  a = Args(); a.host = nullptr;   expect("null images_host", call(a), SNERF_ERR_NULL, "null");
  a = Args(); a.dev = nullptr;    expect("null images_dev", call(a), SNERF_ERR_NULL, "null");
  a = Args(); a.rgbs = nullptr;   expect("null rgbs", call(a), SNERF_ERR_NULL, "null");
  a = Args(); a.sum = nullptr;    expect("null sum", call(a), SNERF_ERR_NULL, "null");
  a = Args(); a.count = nullptr;  expect("null count", call(a), SNERF_ERR_NULL, "null");
  a = Args(); a.stats = nullptr;  expect("null stats", call(a), SNERF_ERR_NULL, "null");
  a = Args(); a.votes = nullptr;  expect("labels without votes", call(a), SNERF_ERR_NULL, "labels and votes");
  a = Args(); a.labels = nullptr; expect("votes without labels", call(a), SNERF_ERR_NULL, "labels and votes");

  SnerfDsmGrid g;
  g = grid; g.res = 0.0;          a = Args(); a.grid = &g; expect("res = 0", call(a), SNERF_ERR_BAD_DESC, "res > 0");
  g = grid; g.res = NAN;          a = Args(); a.grid = &g; expect("res = NaN", call(a), SNERF_ERR_BAD_DESC, "res > 0");
  g = grid; g.xoff = INFINITY;    a = Args(); a.grid = &g; expect("xoff = inf", call(a), SNERF_ERR_BAD_DESC, "res > 0");
  g = grid; g.out_w = 0;          a = Args(); a.grid = &g; expect("out_w = 0", call(a), SNERF_ERR_BAD_DESC, "positive sizes");
  g = grid; g.ysize = -1;         a = Args(); a.grid = &g; expect("ysize = -1", call(a), SNERF_ERR_BAD_DESC, "positive sizes");
  g = grid; g.ioff = INT_MAX - 2; a = Args(); a.grid = &g; expect("window beyond int32", call(a), SNERF_ERR_BAD_DESC, "int32");
  g = grid; g.out_w = 1 << 16; g.out_h = 1 << 15; a = Args(); a.grid = &g; expect("2^31 cells", call(a), SNERF_ERR_BAD_DESC, "2^31");

  a = Args(); a.n_images = 0;                          expect("n_images = 0", call(a), SNERF_ERR_BAD_DESC, "n_images = 0");
  a = Args(); a.n_images = SNERF_RECT_MAX_IMAGES + 1;  expect("n_images = 65", call(a), SNERF_ERR_BAD_DESC, "n_images = 65");
  a = Args(); a.n_classes = 0;                         expect("n_classes = 0", call(a), SNERF_ERR_BAD_DESC, "n_classes = 0");
  a = Args(); a.n_classes = 256;                       expect("n_classes = 256", call(a), SNERF_ERR_BAD_DESC, "n_classes = 256");
  a = Args(); a.n_rows = 0;                            expect("n_rows = 0", call(a), SNERF_ERR_BAD_DESC, "n_rows");
  a = Args(); a.lon0 = 3.2;                            expect("lon0 = 3.2", call(a), SNERF_ERR_BAD_DESC, "central meridian");
  a = Args(); a.lon0 = NAN;                            expect("lon0 = NaN", call(a), SNERF_ERR_BAD_DESC, "central meridian");
  a = Args(); a.south = 2;                             expect("south = 2", call(a), SNERF_ERR_BAD_DESC, "south = 2");

  const SnerfRectImage keep = images[1];
  images[1].w = 0;                 expect("an image with w = 0", call(Args()), SNERF_ERR_BAD_DESC, "image 1 has a bad size");
  images[1] = keep; images[1].h = -3;
  expect("an image with h = -3", call(Args()), SNERF_ERR_BAD_DESC, "image 1 has a bad size");
  images[1] = keep; images[1].row0 = -1;
  expect("an image with row0 = -1", call(Args()), SNERF_ERR_BAD_DESC, "image 1: rows");
  images[1] = keep; images[1].row0 = 21;
  expect("an image one row beyond n_rows", call(Args()), SNERF_ERR_BAD_DESC, "image 1: rows");
  images[1] = keep; images[1].row0 = LLONG_MAX - 3;
  expect("row0 + w * h overflows", call(Args()), SNERF_ERR_BAD_DESC, "image 1: rows");
  images[1] = keep; images[1].rpc.lon_scale = 0.0;
  expect("a zero RPC scale", call(Args()), SNERF_ERR_BAD_DESC, "RPC 1 has a zero");
  images[1] = keep; images[1].rpc.alt_scale = NAN;
  expect("a NaN RPC scale", call(Args()), SNERF_ERR_BAD_DESC, "RPC 1 has a zero");
  images[1] = keep;
  // with labels = votes = NULL the class count is not read
  a = Args(); a.labels = nullptr; a.votes = nullptr; a.n_classes = 0; a.n_images = 0;
  expect("no labels: n_classes unread, n_images = 0 refused", call(a), SNERF_ERR_BAD_DESC, "n_images = 0");

  bool written = stats[0] || stats[1] || stats[2] || stats[3];
  for (int k = 0; k < 12; ++k) written = written || count[k] || sum[k] || votes[k] || state_out[k] || label_out[k] || rgb_out[k] != 0.f || col_row[k] != 0.0;
  if (written) { printf("outputs were written\n"); ++failures; }
  return verdict("orthorect");
}
