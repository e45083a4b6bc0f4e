// recfile_host.cpp -- fpx_recfile.hpp on the host alone: writes the files tests/test_recfile.py compares byte for byte and
// prints what the failure cases reported.  Usage: recfile_host <directory>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../flexpart_amd/csrc/fpx_recfile.hpp"

using fpx::RecFile;

// the four records of one compressed dump of concoutput: count, indices, count, values
static void dump(RecFile &f, const std::vector<int32_t> &idx, const std::vector<float> &val) {
  f.scalar((int32_t)idx.size());
  f.record(idx.data(), idx.size() * 4);
  f.scalar((int32_t)val.size());
  f.record(val.data(), val.size() * 4);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const std::string dir = std::string(argv[1]) + "/";
  bool all = true;
  {
    RecFile f((dir + "empty.bin").c_str());
    f.record(nullptr, 0);
    all = f.close() && all;
  }
  {
    RecFile f((dir + "four.bin").c_str());
    f.scalar((int32_t)3600);
    all = f.close() && all;
  }
  {
    RecFile f((dir + "mixed.bin").c_str());
    f.put((int32_t)-999);
    f.put(999.f);
    f.end();
    f.put((int32_t)5);          // the assembly buffer starts empty again
    f.end();
    all = f.close() && all;
  }
  {
    std::vector<float> r(1000);
    for (int i = 0; i < 1000; i++) r[i] = 0.5f * (float)i;
    RecFile g((dir + "reals.bin").c_str());
    RecFile f(std::move(g));    // the new owner writes and closes; the old one holds nothing
    f.record(r.data(), r.size() * 4);
    all = f.is_open() && !g.is_open() && !g.close() && f.close() && all;
  }
  {
    RecFile f((dir + "conc.bin").c_str());
    f.scalar((int32_t)7200);
    dump(f, {}, {});
    dump(f, {33, 37}, {1.f, 2.f, -3.f, 4.f, 5.f});
    all = f.close() && all;
  }
  {
    RecFile f((dir + "plain.bin").c_str());
    f.write("abc", 3);          // no markers
    all = f.close() && all;
    RecFile a((dir + "plain.bin").c_str(), "ab");
    a.write("de", 2);
    all = a.close() && all;
  }
  printf("written %d\n", (int)all);
  {
    RecFile f((dir + "no_such_directory/x.bin").c_str());
    const bool open = f.is_open();
    f.scalar((int32_t)1);
    printf("nodir open=%d ok=%d close=%d\n", (int)open, (int)f.ok(), (int)f.close());
  }
  {
    RecFile f("/dev/full");
    if (!f.is_open()) printf("devfull absent\n");
    else {
      std::vector<float> r(1000, 1.f);
      f.record(r.data(), r.size() * 4);
      const bool c = f.close();
      printf("devfull close=%d again=%d\n", (int)c, (int)f.close());
    }
  }
  return 0;
}
