// The owning buffer types of the context (csrc/rope_buffers.h) over malloc: a program of its own, built with AddressSanitizer
// and UBSan by tests/test_buffers_host.py.  One line per check; the first that fails ends it with status 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

#include "../rope_s3d_amd/csrc/rope_buffers.h"

namespace {
std::map<void *, size_t> live;                      // block -> bytes
int n_alloc = 0, n_free = 0, fail_next = 0, bad_free = 0;
int seq = 0, last_alloc_seq = 0, last_free_seq = 0; // the order of the calls

int do_alloc(void **p, size_t bytes)
{
    n_alloc++; last_alloc_seq = ++seq;
    *p = nullptr;
    if (fail_next > 0) { fail_next--; return 2; }   // "out of memory"
    *p = std::malloc(bytes ? bytes : 1);
    if (!*p) return 2;
    live[*p] = bytes;
    return 0;
}

int do_free(void *p)
{
    n_free++; last_free_seq = ++seq;
    if (!live.erase(p)) { bad_free++; return 1; }   // not a live block: freed twice, or never allocated
    std::free(p);
    return 0;
}

void check(bool ok, const char *what)
{
    std::printf("%s: %s\n", ok ? "ok" : "FAILED", what);
    if (!ok) std::exit(1);
}
}  // namespace

int rope_dev_alloc(void **p, size_t bytes) { return do_alloc(p, bytes); }
int rope_dev_free(void *p) { return do_free(p); }
int rope_pinned_free(void *p) { return do_free(p); }
int rope_pinned_alloc(void **p, size_t bytes, void **dev_alias)
{
    const int e = do_alloc(p, bytes);
    if (dev_alias) *dev_alias = e ? nullptr : static_cast<char *>(*p) + 1;      // an alias that is recognisably not the host pointer
    return e;
}

template <typename Buf>
static void exercise(const char *kind)
{
    std::printf("-- %s\n", kind);
    const int a0 = n_alloc, f0 = n_free;
    {
        Buf b;
        check(b.get() == nullptr && b.cap() == 0 && !b, "starts empty");
        check(b.grow(10) == 0 && b.get() && b.cap() == 10 && live.at(b.get()) == 10 * sizeof(double) && n_alloc == a0 + 1 && n_free == f0, "grow from empty");
        for (size_t i = 0; i < 10; i++) b.get()[i] = (double)i;                 // the whole block is ours (ASan)
        double *p = b.get();
        check(b.grow(10) == 0 && b.grow(3) == 0 && b.grow(0) == 0 && b.get() == p && b.cap() == 10 && n_alloc == a0 + 1 && n_free == f0,
              "no-op grow: same pointer, no allocator call");
        check(b.grow(11) == 0 && b.cap() == 11 && n_alloc == a0 + 2 && n_free == f0 + 1 && live.count(p) == 0 && last_free_seq < last_alloc_seq,
              "larger grow: the old block freed once, before the new one is allocated");
        b.get()[10] = 1.0;
        fail_next = 1;
        check(b.grow(100) != 0 && b.get() == nullptr && b.cap() == 0 && n_free == f0 + 2 && live.empty(), "failing allocator: empty, the old block gone");
        check(b.grow(4) == 0 && b.get() && b.cap() == 4, "a later grow succeeds");
        p = b.get();
        check(b.reset(4) == 0 && b.cap() == 4 && live.count(p) == 0 && live.size() == 1, "reset: a new block of the same size");

        Buf c;
        check(c.grow(7) == 0, "second buffer");
        double *pb = b.get(), *pc = c.get();
        b.swap(c);
        check(b.get() == pc && b.cap() == 7 && c.get() == pb && c.cap() == 4, "swap: pointer and capacity travel together");
        c.swap(b);
        check(b.get() == pb && b.cap() == 4 && c.get() == pc && c.cap() == 7, "swap back, from the other side");
        Buf empty;
        b.swap(empty);
        check(b.get() == nullptr && b.cap() == 0 && empty.get() == pb && empty.cap() == 4, "swap with an empty buffer");

        Buf m(std::move(c));
        check(m.get() == pc && m.cap() == 7 && c.get() == nullptr && c.cap() == 0, "move construction leaves the source empty");
        const int f1 = n_free;
        empty = std::move(m);
        check(empty.get() == pc && empty.cap() == 7 && m.get() == nullptr && n_free == f1 + 1 && live.count(pb) == 0, "move assignment frees what was held");

        empty.release();
        const int f2 = n_free;
        empty.release();
        check(empty.get() == nullptr && empty.cap() == 0 && n_free == f2 && live.empty(), "release twice");
        check(b.grow(5) == 0 && c.grow(6) == 0 && live.size() == 2, "two blocks left to the destructors");
    }
    check(live.empty() && bad_free == 0, "destructors: no live block, no bad free");
}

int main()
{
    exercise<rope::DevBuf<double>>("DevBuf");
    exercise<rope::PinnedBuf<double>>("PinnedBuf");
    {
        rope::PinnedBuf<int32_t> plain, mapped(true);
        check(plain.grow(8) == 0 && plain.dev() == nullptr, "PinnedBuf, not mapped: no device alias");
        check(mapped.grow(8) == 0 && mapped.dev() == reinterpret_cast<int32_t *>(reinterpret_cast<char *>(mapped.get()) + 1), "PinnedBuf, mapped: the allocator's alias");
        int32_t *alias = mapped.dev();
        rope::PinnedBuf<int32_t> other(true);
        other.swap(mapped);
        check(other.dev() == alias && mapped.dev() == nullptr && mapped.get() == nullptr, "the alias travels with the block");
        other.release();
        check(other.dev() == nullptr, "release drops the alias");
        fail_next = 1;
        check(other.grow(8) != 0 && other.get() == nullptr && other.dev() == nullptr && other.cap() == 0, "failing allocator: no alias either");
    }
    check(live.empty() && bad_free == 0, "nothing live at exit");
    return 0;
}
