// Stand-alone host program (its own main; no HIP, no device): the prefixed parser (host/prefix.hpp), the scanner's fifth dialect
// (host/boolean.hpp) and the prefix-aware tokenizer (host/term_dict.hpp for_each_star_term) on the cases of tests/test_prefix_cpu.py,
// built there with -fsanitize=address,undefined and run on the CPU.  Exit status 0 and "prefix host check OK" when every
// expectation holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "prefix.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static std::string weight_text(float w) {
    char buf[32];
    std::snprintf(buf, sizeof(buf), "%g", (double)w);
    return buf;
}

// term[*]:role clause/need [p] ^weight, then ~min_should
static std::string shown(const std::string& text) {
    uint32_t m = 0;
    std::string o;
    for (const nsx::PrefixedTerm& t : nsx::parse_prefixed(text, &m))
        o += t.text + (t.prefix ? "*" : "") + ":" + "SMX"[t.role] + std::to_string(t.clause) + "/" + std::to_string(t.need) + (t.promoted ? "p" : "") + "^" + weight_text(t.weight) + " ";
    return o + "~" + std::to_string(m);
}

static void parser() {
    EXPECT(shown("vaccin*") == "vaccin*:S0/0^1 ~0");
    EXPECT(shown("+vaccin*") == "vaccin*:M0/1^1 ~0");
    EXPECT(shown("-mouse*") == "mouse*:X0/0^1 ~0");
    EXPECT(shown("+(vaccin* immun*)~1") == "vaccin*:M0/1^1 immun*:M0/1^1 ~0");
    EXPECT(shown("vir*^2.5") == "vir*:S0/0^2.5 ~0");
    EXPECT(shown("vac*cine") == "vac:S0/0^1 cine:S0/0^1 ~0");                 // a '*' with an alphanumeric byte behind it separates
    EXPECT(shown("a*") == "~0");                                              // shorter than 2 bytes
    EXPECT(shown("the*") == "the*:S0/0^1 ~0" && shown("the") == "~0");       // no stop-word test on a prefix
    EXPECT(shown("covid-19*") == "covid:S0/0^1 19*:S0/0^1 ~0");
    EXPECT(shown("**") == "~0" && shown("*") == "~0" && shown("x *") == "~0" && shown("ab *") == "ab:S0/0^1 ~0");
    EXPECT(shown("VacCin*") == "vaccin*:S0/0^1 ~0");                          // lower-cased
    EXPECT(shown("vaccin** immun*.") == "vaccin*:S0/0^1 immun*:S0/0^1 ~0");
    EXPECT(shown("vaccin*,safety*") == "vaccin*:S0/0^1 safety*:S0/0^1 ~0");
    EXPECT(shown("+(vaccin* immun*)~1 trial^2") == "vaccin*:M0/1^1 immun*:M0/1^1 trial:S0/0^2 ~0");
    EXPECT(shown("vir*^0.5 vir*") == "vir*:S0/0^0.5 vir*:S0/0^1 ~0");
    EXPECT(shown("+(vir* cov*)^3 -(mouse* rat)^2") == "vir*:M0/1^3 cov*:M0/1^3 mouse*:X0/0^1 rat:X0/0^1 ~0");
    EXPECT(shown("vir* cov* ~1") == "vir*:M0/1p^1 cov*:M0/1p^1 ~1");
    EXPECT(shown("vir*^") == "vir*:S0/0^1 ~0" && shown("vir*^x") == "vir*:S0/0^1 ~0");   // no weight: the '^' is not alphanumeric either
    EXPECT(shown("vir*2") == "vir:S0/0^1 ~0");                                           // "2" is a one-byte token
    // a text without such a '*' is parse_boosted's
    for (const char* text : {"+(coronavirus covid sars)^0.5 +(vaccine vaccination) -mouse safety^2", "+(a1 b1 c1)~2", "a1 b1 c1 ~2", "+d1 a1 (b1 c1)~2^3 -e1 ~1", "+(alpha beta", "+(",
                             "~", "(", ")~2", "+()~3", "a~2", "+(a1)~2~3", "~99999999999999999999 a1", "", "vac*cine the of", "ab^1e3", "x *y"}) {
        uint32_t mb = 0, mp = 0;
        const std::vector<nsx::BoostedTerm> b = nsx::parse_boosted(text, &mb);
        const std::vector<nsx::PrefixedTerm> p = nsx::parse_prefixed(text, &mp);
        EXPECT(b.size() == p.size() && mb == mp);
        for (size_t i = 0; i < b.size() && i < p.size(); i++)
            EXPECT(b[i].text == p[i].text && b[i].role == p[i].role && b[i].clause == p[i].clause && b[i].need == p[i].need && b[i].promoted == p[i].promoted &&
                   b[i].weight == p[i].weight && !p[i].prefix);
    }
    // every prefix of a text with every form, each an exact-size heap copy: the scanner never reads past the end, whether the cut
    // falls behind a '*', inside a weight or behind a ')'
    const std::string all = "+(vaccin* b1)~2^1.5 -(c1*)~3^2 (d1 e1*)^0.25 f1*^3 ~2 +g1*^2.5 vac*cine h1* ** j1*";
    for (size_t n = 0; n <= all.size(); n++) {
        std::vector<char> exact(all.begin(), all.begin() + n), scratch;
        size_t terms = 0, stars = 0;
        nsx::for_each_prefixed_term(exact.data(), exact.size(), scratch, [&](const char* p, size_t len, uint8_t, uint32_t, uint32_t, float w, bool star) {
            terms++;
            stars += star;
            EXPECT(len >= 2 && w > 0.0f && w <= 1e6f);
            for (size_t i = 0; i < len; i++) EXPECT((p[i] >= 'a' && p[i] <= 'z') || (p[i] >= '0' && p[i] <= '9'));
        });
        EXPECT(n < 9 || terms >= 1);
        EXPECT(n < all.size() || stars == 7);
    }
    // the tokenizer alone, on exact-size copies of the shortest texts
    for (const char* text : {"", "*", "a", "a*", "ab", "ab*", "ab*c", "ab**", "*ab", "ab* ", "ab *", "the*", "the"}) {
        std::vector<char> exact(text, text + std::strlen(text)), scratch;
        std::string got;
        nsx::for_each_star_term(exact.data(), exact.size(), scratch, [&](const char* p, size_t len, bool star) { got += std::string(p, len) + (star ? "* " : " "); });
        const std::string t(text);
        const std::string want = (t == "ab" || t == "*ab" || t == "ab *") ? "ab " : (t == "ab*" || t == "ab**" || t == "ab* ") ? "ab* " : t == "ab*c" ? "ab " : t == "the*" ? "the* " : "";
        EXPECT(got == want);
    }
}

int main() {
    parser();
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("prefix host check OK");
    return 0;
}
