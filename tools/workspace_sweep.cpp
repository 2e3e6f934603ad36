// tools/workspace_sweep.cpp -- the plan of the whole path's workspace (ek_solve.hip plan_path) for every order from 1 to
// 40000, through the ek_hip_debug_*workspace_bytes entries: host arithmetic only, no GPU.  Meant for a build of the host
// code with a sanitizer, on the CPU:
//   cd eigenkernel_amd/csrc && make
//   hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -c ek_solve.hip -o /tmp/ek_solve_san.o
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -I../../include -c ../../tools/workspace_sweep.cpp -o /tmp/sweep.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/sweep.o /tmp/ek_solve_san.o \
//         $(ls ek_*.o | grep -v '^ek_solve.o$') -o /tmp/workspace_sweep
//   /tmp/workspace_sweep
// Prints the number of plans and a checksum of their sizes (the same for every build that plans alike).
#include <cstdio>

#include "ek_hip.h"
#include "ek_hip_debug.h"

int main() {
  unsigned long long sum = 0, plans = 0, parts[6];
  for (int n = 1; n <= 40000; ++n) {
    for (int problem = 0; problem < 2; ++problem) {
      const int m = n < 64 ? n : 64;
      sum += ek_hip_debug_workspace_bytes(problem, n, n, 1, parts);
      sum += ek_hip_debug_workspace_bytes(problem, n, m, 8, parts) + parts[4];
      sum += ek_hip_debug_values_workspace_bytes(problem, n);
      for (int jobz = 0; jobz < 2; ++jobz)
        for (int range = 0; range < 2; ++range) sum += ek_hip_debug_window_workspace_bytes(problem, n, jobz, range, m);
      plans += 7;
    }
    for (int itype = 1; itype <= 3; ++itype) sum += ek_hip_debug_sygvx_workspace_bytes(itype, n, 1, 0, n);
    plans += 3;
  }
  printf("%llu plans, checksum %llu\n", plans, sum);
  return 0;
}
