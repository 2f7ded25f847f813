// subscribe_host_baseline.cpp -- the host side of scripts/subscribe_route_measure.py: a burst of
// Subscribes answered by one thread, the shape of the reference's one task per connection
// (publisher/server.rs:60-137): a by_path hash lookup on the path string, a by_id lookup, and one
// From::Subscribed(path, id, current) encoded per message with the library's host encoder
// nxg_msg_subscribed.
//
//   subscribe_host_baseline <libnxg_codec.so> <paths file> <reps>
// paths file: u64 n, u64 off[n + 1], the bytes. Path i maps to Id i, whose current value is the
// F64 with bit pattern i. Prints one JSON line: the median wall time of a pass over the burst.
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

typedef int64_t (*msg_subscribed_fn)(const char*, uint64_t, uint64_t, uint8_t, uint64_t, uint32_t,
                                     const uint8_t*, uint8_t*, uint64_t);

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) {
        fprintf(stderr, "%s\n", dlerror());
        return 1;
    }
    msg_subscribed_fn enc = (msg_subscribed_fn)dlsym(lib, "nxg_msg_subscribed");
    FILE* f = fopen(argv[2], "rb");
    if (!enc || !f) return 1;
    uint64_t n = 0;
    if (fread(&n, 8, 1, f) != 1) return 1;
    std::vector<uint64_t> off(n + 1);
    if (fread(off.data(), 8, n + 1, f) != n + 1) return 1;
    std::vector<char> bytes(off[n]);
    if (fread(bytes.data(), 1, off[n], f) != off[n]) return 1;
    fclose(f);
    const int reps = atoi(argv[3]);
    std::unordered_map<std::string, uint64_t> by_path;
    std::unordered_map<uint64_t, uint64_t> by_id;  // Id -> current (an F64's bits)
    by_path.reserve(n);
    by_id.reserve(n);
    for (uint64_t i = 0; i < n; i++) {
        by_path.emplace(std::string(bytes.data() + off[i], off[i + 1] - off[i]), i);
        by_id.emplace(i, i);
    }
    std::vector<uint8_t> reply(off[n] + n * 32);
    std::vector<double> ms;
    uint64_t len = 0, found = 0;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        len = found = 0;
        // the burst in another order than the table was built in, as a subscriber's is
        for (uint64_t j = 0; j < n; j++) {
            const uint64_t i = (j * 7919) % n;
            const std::string path(bytes.data() + off[i], off[i + 1] - off[i]);  // Path::decode
            const auto it = by_path.find(path);
            if (it == by_path.end()) continue;
            const auto cur = by_id.find(it->second);
            if (cur == by_id.end()) continue;
            const int64_t m = enc(path.data(), path.size(), it->second, 9, cur->second, 0, nullptr,
                                  reply.data() + len, reply.size() - len);
            if (m < 0) return 1;
            len += (uint64_t)m;
            found++;
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                         .count());
    }
    std::sort(ms.begin(), ms.end());
    printf("{\"host_subscribes\": %llu, \"host_found\": %llu, \"host_reply_bytes\": %llu, "
           "\"host_reps\": %d, \"host_ms\": %.3f}\n",
           (unsigned long long)n, (unsigned long long)found, (unsigned long long)len, reps,
           ms[ms.size() / 2]);
    return 0;
}
