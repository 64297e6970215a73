/* Exhaustive check of csrc/exact_math.h glibc_powf against libm powf: every positive float bit
 * pattern up to 1.0f (subnormals included) at y = 1.0f / T for the T of tests/test_powf_exact.py.
 * Build (host code only; the HIP header supplies __host__ __device__):
 *   hipcc -O2 -ffp-contract=on -x hip --cuda-host-only tools/powf_sweep.c -o powf_sweep -lpthread
 * Prints the mismatch count per y; 0 everywhere is recorded in DESIGN.md section 22. */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../rwkv-tts-rs_amd/csrc/exact_math.h"

static const float kT[12] = {0.1f, 0.25f, 0.5f, 0.7f, 0.8f, 0.9f, 1.1f, 1.25f, 1.5f, 2.0f, 3.0f, 4.0f};
static long g_mism[12];

static void* run(void* arg) {
  const int j = (int)(intptr_t)arg;
  const float y = 1.0f / kT[j];
  long mism = 0;
  for (uint32_t u = 1; u <= 0x3F800000u; ++u) {
    float x, a, b;
    memcpy(&x, &u, 4);
    a = rwkvtts::glibc_powf(x, y);
    b = powf(x, y);
    if (memcmp(&a, &b, 4) != 0) {
      if (mism < 3) printf("T=%g x=%a libm=%a restated=%a\n", (double)kT[j], (double)x, (double)b, (double)a);
      ++mism;
    }
  }
  g_mism[j] = mism;
  return 0;
}

int main() {
  pthread_t th[12];
  for (int j = 0; j < 12; ++j) pthread_create(&th[j], 0, run, (void*)(intptr_t)j);
  long total = 0;
  for (int j = 0; j < 12; ++j) {
    pthread_join(th[j], 0);
    printf("T=%g y=%a mismatches=%ld of %u\n", (double)kT[j], (double)(1.0f / kT[j]), g_mism[j], 0x3F800000u);
    total += g_mism[j];
  }
  printf("total mismatches=%ld\n", total);
  return total != 0;
}
