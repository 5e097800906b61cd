// tools/check_sharded.cpp -- drives csrc/host/sharded.h (the rank protocol of the sharded searches) through a fake all-reduce, for
// a world of one and a world of two: two Sharded objects whose vectors are max-merged by hand.  Plain host C++, meant for
//   g++ -std=c++17 -g -fsanitize=address,undefined -Iinclude -Ilinear_programming_solver_lpr381_amd/csrc/host tools/check_sharded.cpp -o check_sharded
// Exit status 0 and "check_sharded ok" when every case holds.
#include "sharded.h"

#include <cstdio>
#include <cstdlib>

using namespace lpx::host;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "check_sharded: line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static double g_peer[16]; static int g_peer_n = 0;         // what the other rank put on the wire this round
static void merge(double* v, int n) { CHECK(n == g_peer_n); for (int i = 0; i < n; ++i) v[i] = std::max(v[i], g_peer[i]); }

static EngineOptions options(int rank, int world, bool shard_one)
{
    EngineOptions o; o.rank = rank; o.world = world; o.shard_one = shard_one;
    o.allreduce_max = world > 1 ? merge : [](double*, int) {};
    return o;
}

// one exchange of rank 0 against a peer whose vector is built by a second object (its own reduce sees only itself)
static Sharded::Round round_of_two(Sharded& a, Sharded& peer, int n, double za, bool work_a, double zb, bool work_b)
{
    std::vector<double> vb(n, -INFINITY), va(n, -INFINITY);
    g_peer_n = n; for (int i = 0; i < n; ++i) g_peer[i] = -INFINITY;
    peer.exchange(vb.data(), n, zb, work_b);                 // merges with -inf: vb is what the peer sent
    for (int i = 0; i < n; ++i) g_peer[i] = vb[i];
    return a.exchange(va.data(), n, za, work_a);
}

int main()
{
    {   // a world of one told to shard: first exchange carries its own fingerprint, then stops when out of work
        EngineOptions o = options(0, 1, true); Sharded s(o, "the node LPs");
        CHECK(s.sharded && !s.replicated && s.exchanging() && s.mine(0) && s.mine(7));
        Fingerprint f(false); f.mix(3); f.mix_bits(1.5); s.agree(f.value());
        CHECK(f.value() >= 0 && f.value() < 4503599627370496.0);
        double v[5] = {0, 0, 0, -INFINITY, -INFINITY};
        Sharded::Round r = s.exchange(v, 5, 7.0, true);
        CHECK(r.verdict == Sharded::GO_ON && !r.better && v[3] == f.value() && v[4] == -f.value() && s.allreduces == 1);
        double w[5] = {0, 0, 0, -INFINITY, -INFINITY};
        r = s.exchange(w, 5, 7.0, false);
        CHECK(r.verdict == Sharded::STOP && w[3] == -INFINITY && !s.failed);
        s.rethrow();
    }
    {   // no collective: not sharded, nothing to send
        EngineOptions o; o.world = 2; Sharded s(o, "the bounds");
        CHECK(!s.sharded && s.replicated && !s.exchanging() && s.agree_sent);
    }
    for (int n : {5, 8}) {   // a world of two, 5 doubles (warm search, knapsack) and 6 + world (cold level search)
        EngineOptions o0 = options(0, 2, false), o1 = options(1, 2, false);
        {   // agreement, a better incumbent on the peer, then termination
            Sharded a(o0, "the node LPs"), b(o1, "the node LPs");
            CHECK(a.sharded && a.replicated && a.mine(0) && !a.mine(1) && b.mine(1));
            a.agree(42.0); b.agree(42.0);
            Sharded::Round r = round_of_two(a, b, n, 3.0, false, 9.0, true);
            CHECK(r.verdict == Sharded::GO_ON && r.better && r.best == 9.0);
            r = round_of_two(a, b, n, 9.0, false, 9.0, false);
            CHECK(r.verdict == Sharded::STOP && !r.better && !a.failed);
        }
        {   // the ranks left the warm-up with different states
            Sharded a(o0, "the bounds"), b(o1, "the bounds");
            a.agree(42.0); b.agree(43.0);
            Sharded::Round r = round_of_two(a, b, n, 1.0, true, 1.0, true);
            CHECK(r.verdict == Sharded::DIVERGED && a.failed && a.fail_code == LPX_EDEVICE);
            CHECK(a.fail_msg.find("(the bounds must be bit-identical across ranks)") != std::string::npos);
            bool thrown = false; try { a.rethrow(); } catch (const LpxException& e) { thrown = e.code == LPX_EDEVICE; }
            CHECK(thrown);
        }
        {   // the peer failed inside the warm-up: it sends no fingerprint, and that is not reported as divergence
            Sharded a(o0, "the node LPs"), b(o1, "the node LPs");
            a.agree(42.0); b.fail(LpxException(LPX_ENOMEM, "out of memory"));
            CHECK(!b.replicated && b.exchanging());
            Sharded::Round r = round_of_two(a, b, n, 1.0, true, -INFINITY, false);
            CHECK(r.verdict == Sharded::PEER_FAILED && a.failed && a.fail_msg == "sharded search: a peer rank failed");
            bool own = false; try { b.rethrow(); } catch (const LpxException& e) { own = e.code == LPX_ENOMEM && std::string(e.what()) == "out of memory"; }
            CHECK(own);
        }
        {   // this rank failed after agreeing: it keeps its own error and stops with the peer
            Sharded a(o0, "the node LPs"), b(o1, "the node LPs");
            a.agree(42.0); b.agree(42.0);
            CHECK(round_of_two(a, b, n, 1.0, true, 1.0, true).verdict == Sharded::GO_ON);
            a.fail(LpxException(LPX_EINVAL, "mine"));
            CHECK(round_of_two(a, b, n, 1.0, false, 1.0, true).verdict == Sharded::PEER_FAILED && a.fail_msg == "mine" && a.fail_code == LPX_EINVAL);
        }
    }
    std::puts("check_sharded ok");
    return 0;
}
