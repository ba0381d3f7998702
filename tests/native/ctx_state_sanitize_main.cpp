// ctx_state.hpp's lazy slot as a stand-alone program for AddressSanitizer / UBSan, with a counting dummy state and a dummy ctx: an
// empty slot, make twice, reset and make again, a slot destroyed while it holds a state, two slots of one struct destroyed in
// reverse order of declaration.  A leak or a double free fails the run through the sanitizer.  Built and run by
// tests/test_ctx_state_host.py; nothing of it runs in the Python process.
#include "ctx_state.hpp"
#include <cstdio>
#include <string>

struct isdf_ctx { std::string err; };
int isdf_fail(isdf_ctx *c, int code, const char *msg) { if (c) c->err = msg; return code; }

namespace {
int failures = 0;
void expect(bool ok, const char *what) { if (!ok) { std::printf("FAILED: %s\n", what); failures++; } }

int made = 0, dropped = 0;
std::string order;
template <char Tag> struct Dummy {
    int *heap = new int[4]{};            // (a skipped destructor is a leak, a second one a double free)
    Dummy() { made++; }
    ~Dummy() { dropped++; order += Tag; delete[] heap; }
};
using A = Dummy<'a'>;
using B = Dummy<'b'>;
struct Two { isdf::Lazy<A> first; isdf::Lazy<B> second; };
}  // namespace

int main() {
    isdf_ctx ctx;
    {
        isdf::Lazy<A> slot;
        expect(!slot && slot.get() == nullptr, "a new slot is empty");
        slot.reset();
    }
    expect(made == 0 && dropped == 0, "an empty slot constructs and destroys nothing");
    std::printf("empty ok: %d made, %d dropped\n", made, dropped);

    {
        isdf::Lazy<A> slot;
        A *p = nullptr, *q = nullptr;
        expect(slot.make(&ctx, &p) == 0 && p && made == 1, "the first make constructs");
        expect(slot.make(&ctx, &q) == 0 && q == p && made == 1, "the second make returns the same object");
        expect(slot.get() == p && (bool)slot, "get returns it");
        slot.reset();
        expect(dropped == 1 && slot.get() == nullptr, "reset destroys exactly once");
        slot.reset();
        expect(dropped == 1, "a second reset destroys nothing");
        expect(slot.make(&ctx, &q) == 0 && q && made == 2, "a make after reset constructs anew");
        std::printf("make / reset ok: %d made, %d dropped\n", made, dropped);
    }
    expect(made == 2 && dropped == 2, "a slot destroyed while holding a state runs its destructor once");
    std::printf("held ok: %d made, %d dropped\n", made, dropped);

    order.clear();
    {
        Two t;
        A *a = nullptr;
        B *b = nullptr;
        expect(t.second.make(&ctx, &b) == 0 && t.first.make(&ctx, &a) == 0, "both slots made, the second first");
    }
    expect(order == "ba", "slots are destroyed in reverse order of declaration");
    expect(made == 4 && dropped == 4 && ctx.err.empty(), "every state made was dropped, no error recorded");
    std::printf("order ok: %s\n", order.c_str());
    return failures ? 1 : 0;
}
