// Stand-in for smithlab_cpp's OptionParser: short (-x) and long (-name, --name) options, with a value (the next argument)
// or without (bool targets), and the leftover arguments.  No help texts: the reference binary built with this is driven
// by tests that give complete command lines.  Our own code.
#pragma once
#include <cstddef>
#include <functional>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

class OptionParser {
public:
  OptionParser(const std::string & /*program*/, const std::string & /*description*/, const std::string & /*arguments*/ = "",
               size_t /*n_leftover*/ = 0) {}
  void set_show_defaults() {}

  void add_opt(const std::string &long_name, char short_name, const std::string & /*help*/, bool required, bool &target) {
    opts.push_back({long_name, short_name, false, required, false, [&target](const std::string &) { target = true; }});
  }

  template <class T>
  void add_opt(const std::string &long_name, char short_name, const std::string & /*help*/, bool required, T &target) {
    opts.push_back({long_name, short_name, true, required, false, [&target, long_name](const std::string &text) {
                      std::istringstream in(text);
                      if (!(in >> target)) throw std::runtime_error("bad value for option " + long_name + ": " + text);
                    }});
  }

  void parse(int argc, char *argv[], std::vector<std::string> &leftover) {
    for (int i = 1; i < argc; ++i) {
      const std::string a = argv[i];
      Opt *hit = nullptr;
      if (a.size() > 1 && a[0] == '-')
        for (Opt &o : opts)
          if (a == std::string("-") + o.short_name || a == "-" + o.long_name || a == "--" + o.long_name) hit = &o;
      if (!hit) {
        leftover.push_back(a);
        continue;
      }
      if (hit->takes_value && i + 1 >= argc) throw std::runtime_error("missing value for option " + a);
      hit->set(hit->takes_value ? argv[++i] : "");
      hit->seen = true;
    }
  }

  bool help_requested() const { return false; }
  bool about_requested() const { return false; }
  bool option_missing() const {
    for (const Opt &o : opts)
      if (o.required && !o.seen) return true;
    return false;
  }
  std::string help_message() const { return "(no help text in this build)"; }
  std::string about_message() const { return ""; }
  std::string option_missing_message() const {
    std::string m;
    for (const Opt &o : opts)
      if (o.required && !o.seen) m += "missing required option: -" + o.long_name + "\n";
    return m;
  }

private:
  struct Opt {
    std::string long_name;
    char short_name;
    bool takes_value, required, seen;
    std::function<void(const std::string &)> set;
  };
  std::vector<Opt> opts;
};
