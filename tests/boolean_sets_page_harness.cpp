// C entry points over host/page.hpp for tests/test_boolean_sets_cpu.py (built by g++ inside the test; no HIP, no device, no
// engine): the cursor kind of every page mode, and parse_cursor / cursor_text under that kind.
#include <cstdint>
#include <cstring>
#include <string>

#include "page.hpp"

extern "C" {

int page_kind_c(int mode) { return (int)nsx::page_kind((nsx::PageSpec::Mode)mode); }
int page_mode_boolean_sorted(void) { return (int)nsx::PageSpec::BooleanSorted; }

// text -> out[0..3] = {set, rank, position, doc} under the kind of `mode`; 0, or -1 with the parser's message in err
int page_parse_c(const char* text, int mode, uint32_t* out, char* err, uint32_t err_cap) {
    nsx::PageCursor c;
    std::string why;
    const bool ok = nsx::parse_cursor(text, nsx::page_kind((nsx::PageSpec::Mode)mode), c, why);
    out[0] = c.set ? 1u : 0u; out[1] = c.rank; out[2] = c.seg; out[3] = c.doc;
    if (err && err_cap) {
        const size_t n = why.size() < err_cap - 1 ? why.size() : err_cap - 1;
        std::memcpy(err, why.data(), n);
        err[n] = 0;
    }
    return ok ? 0 : -1;
}

// the text form of {rank, position, doc} under the kind of `mode`, NUL-terminated into buf (cap >= 32)
void page_text_c(int mode, uint32_t rank, uint32_t pos, uint32_t doc, char* buf, uint32_t cap) {
    nsx::PageCursor c;
    c.set = true; c.rank = rank; c.seg = pos; c.doc = doc;
    const std::string t = nsx::cursor_text(nsx::page_kind((nsx::PageSpec::Mode)mode), c);
    const size_t n = t.size() < cap - 1 ? t.size() : cap - 1;
    std::memcpy(buf, t.data(), n);
    buf[n] = 0;
}

}  // extern "C"
