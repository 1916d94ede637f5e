// cli_opts_check.cpp — sw_cli.cpp (main's flags and their checks) against
// tests/golden/cli_flag_cases.json, recorded from the main that checked its
// flags inline (tests/golden/record_cli_flag_cases.py): for every argument
// list the exit code, stdout and stderr that main decided before it touched
// the library.  Links sw_cli.cpp alone.
//
// A case the flags' checks pass was decided by the next step, reading an
// input file that does not exist: then the recorded stderr must be that
// file's "cannot open" text and nothing else.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "sw_cli.h"

namespace {

// The JSON of the fixture: objects, arrays, strings and integers.
struct Json {
    const std::string& s;
    size_t at = 0;

    [[noreturn]] void fail(const char* why) const {
        std::fprintf(stderr, "cli_flag_cases.json: %s at byte %zu\n", why, at);
        std::exit(2);
    }
    void space() {
        while (at < s.size() && (s[at] == ' ' || s[at] == '\n' || s[at] == '\t' || s[at] == '\r')) ++at;
    }
    bool take(char c) {
        space();
        if (at < s.size() && s[at] == c) return ++at, true;
        return false;
    }
    void need(char c) {
        if (!take(c)) fail("unexpected character");
    }
    std::string string() {
        need('"');
        std::string out;
        while (at < s.size() && s[at] != '"') {
            char c = s[at++];
            if (c == '\\') {
                if (at >= s.size()) fail("unfinished escape");
                c = s[at++];
                if (c == 'n') c = '\n';
                else if (c == 't') c = '\t';
                else if (c != '"' && c != '\\' && c != '/') fail("unsupported escape");
            }
            out += c;
        }
        if (at >= s.size()) fail("unfinished string");
        ++at;
        return out;
    }
    int integer() {
        space();
        char* end = nullptr;
        const long v = std::strtol(s.c_str() + at, &end, 10);
        if (end == s.c_str() + at) fail("expected an integer");
        at = static_cast<size_t>(end - s.c_str());
        return static_cast<int>(v);
    }
};

struct Case {
    std::vector<std::string> args;
    int code = -1;
    std::string out, err;
};

Case read_case(Json& j) {
    Case c;
    j.need('{');
    do {
        const std::string key = j.string();
        j.need(':');
        if (key == "args") {
            j.need('[');
            if (!j.take(']')) {
                do c.args.push_back(j.string());
                while (j.take(','));
                j.need(']');
            }
        } else if (key == "code") c.code = j.integer();
        else if (key == "stdout") c.out = j.string();
        else if (key == "stderr") c.err = j.string();
        else j.fail("unknown key");
    } while (j.take(','));
    j.need('}');
    return c;
}

std::string show(const Case& c) {
    std::string s = "main";
    for (const std::string& a : c.args) s += " " + a;
    return s;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: cli_opts_check cli_flag_cases.json\n"), 2;
    std::ifstream in(argv[1]);
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (text.empty()) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    Json j{text};
    std::string usage;
    std::vector<Case> cases;
    j.need('{');
    do {
        const std::string key = j.string();
        j.need(':');
        if (key == "usage") usage = j.string();
        else if (key == "cases") {
            j.need('[');
            do cases.push_back(read_case(j));
            while (j.take(','));
            j.need(']');
        } else j.fail("unknown key");
    } while (j.take(','));
    j.need('}');

    int bad = 0, by_flags = 0, by_inputs = 0;
    if (usage != swcli::usage_text()) ++bad, std::printf("the usage text differs from the recorded one\n");
    for (const Case& c : cases) {
        std::vector<const char*> av{"main"};
        for (const std::string& a : c.args) av.push_back(a.c_str());
        swcli::Options o;
        swcli::Verdict v = swcli::parse(static_cast<int>(av.size()), av.data(), &o);
        if (v.what == swcli::Verdict::PROCEED) v = swcli::validate(o);
        int code = -1;
        std::string out, err;
        if (v.what == swcli::Verdict::STOP && !v.after_matrix) {
            ++by_flags;
            code = v.code;
            err = v.err;
            out = v.usage ? "@usage" : "";
        } else if (v.what == swcli::Verdict::PROCEED && !o.custom() && (o.pssm.set || o.queries.set)) {
            ++by_inputs;
            code = 1;
            err = o.pssm.set ? "--pssm " + o.pssm.text + ": cannot open PSSM file\n"
                             : "--queries " + o.queries.text + ": cannot open query file\n";
        } else {
            // --make-db, a matrix to read, a query to scan: main goes to the library
            err = "(the flags pass to the library: no such case is recorded)";
        }
        if (code != c.code || out != c.out || err != c.err) {
            ++bad;
            std::printf("%s\n  recorded: exit %d stdout '%s' stderr '%s'\n  now:      exit %d stdout '%s' stderr '%s'\n",
                        show(c).c_str(), c.code, c.out.c_str(), c.err.c_str(), code, out.c_str(), err.c_str());
        }
    }
    std::printf("cases %zu: %d decided by the flags, %d by a missing input file, %d differ\n", cases.size(), by_flags,
                by_inputs, bad);
    if (bad) return 1;
    std::printf("cli_opts_check ok\n");
    return 0;
}
